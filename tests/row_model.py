"""Exact integer model of the 29-bit engine's row and quad field layers (csrc/row29.h RowF, the Q29
policy of csrc/assemble.hip) and of the point formulas written over them (quad_dbl, quad_add, the
negation in glv_row_mul), for tests/test_row_bounds_cpu.py and tests/test_gpu_asm_arith.py.

A row is a list of 16 lanes (u32), lane j < 9 holding limb j; a quad value is a list of 9 limbs.
Limbs are LAZY: lanes 0..7 below LAZY = 2^29 + 2^7, lane 8 the exact top.  value() is the unsigned
limb sum, the integer every operation is specified on.
"""
from oracle import bn254 as bn

Q = bn.Q                      # the modulus of P29
B = 29
MASK = (1 << B) - 1
LAZY = (1 << B) + (1 << 7)    # exclusive bound of a lazy limb (lanes 0..7)
R261 = 1 << (9 * B)
NINV = (-pow(Q, -1, 1 << B)) % (1 << B)
U32 = (1 << 32) - 1
U64 = (1 << 64) - 1
ONE = R261 % Q                # the Montgomery form of 1
_QINV = pow(Q, -1, R261)

# row_kp's bias (row29.h): + KP_HI on lanes 0..7, - KP_LO on lanes 1..8; KP_HI 2^(29 j) summed over
# lanes 0..7 equals KP_LO 2^(29 j) summed over lanes 1..8, so the limb sum stays K M
KP_HI = 1 << 31
KP_LO = 4


def limbs(x, n=9):
    """normalized limbs of x >= 0: limbs 0..n-2 below 2^29, the last holds the rest"""
    return [(x >> (B * i)) & MASK for i in range(n - 1)] + [x >> (B * (n - 1))]


def value(l):
    return sum(int(v) << (B * i) for i, v in enumerate(l[:9]))


def row(l):
    return [int(v) for v in l[:9]] + [0] * 7


def lazy_spread(x):
    """x's limbs with every lower limb that can take it raised by 2^29 (the next lowered by one):
    the same integer in the lazy form, limbs 0..7 still below LAZY"""
    l = limbs(x)
    for i in range(8):
        if l[i] < (1 << 7) and l[i + 1] > 0:
            l[i] += 1 << B
            l[i + 1] -= 1
    assert value(l) == x and all(0 <= v < LAZY for v in l[:8])
    return l


def lazy_limb(rnd):
    """a random lazy limb: half of them in the band above 2^29 that only carry-save steps produce
    (a uniform draw below 2^29 + 2^7 lands there once in 2^22), some at the band's ends"""
    u = rnd.random()
    if u < 0.5:
        return rnd.randrange(1 << B, LAZY)
    if u < 0.75:
        return rnd.randrange(LAZY)
    return rnd.choice((0, MASK, 1 << B, LAZY - 1))


def kp_limbs(k, m=Q):
    return limbs(k * m)


def row_kp(k, m=Q, hi=KP_HI, lo=KP_LO):
    r = kp_limbs(k, m)
    return [(r[i] + (hi if i < 8 else 0) - (lo if i > 0 else 0)) & U32 for i in range(9)] + [0] * 7


def borrowed(k, m=Q):
    """p29_times(k, true): every lower limb raised by 2^29, the next lowered by one"""
    r = kp_limbs(k, m)
    for i in range(8):
        r[i] += (1 << B) - (1 if i else 0)
    r[8] -= 1
    return r


# ---------------------------------------------------------------------------
# RowF
# ---------------------------------------------------------------------------
def carry(x):
    h = [x[j] >> B if j < 8 else 0 for j in range(16)]
    return [((x[j] & MASK if j < 8 else x[j]) + (h[j - 1] if j else 0)) & U32 for j in range(16)]


def row_add(a, b):
    return carry([(a[j] + b[j]) & U32 for j in range(16)])


def row_sub(k, a, b, m=Q, hi=KP_HI, lo=KP_LO):
    kp = row_kp(k, m, hi, lo)
    return carry([(a[j] + kp[j] - b[j]) & U32 for j in range(16)])


def row_sub_lanes_in_range(k, a, b, m=Q, hi=KP_HI, lo=KP_LO):
    """no lane 0..7 of a + row_kp - b leaves [0, 2^32) (lane 8 may: the carries make it whole)"""
    kp = kp_limbs(k, m)
    return all(0 <= a[j] + kp[j] + hi - (lo if j else 0) - b[j] <= U32 for j in range(8))


def row_mont(a, b, m=Q):
    """RowF::mont<K>: a = K operands of 9 limbs (replicated), b = K rows -> the row, lane by lane as
    the kernel computes it (64-bit columns, the row shifted down one lane per reduction digit)"""
    pl = limbs(m) + [0] * 7
    ninv = (-pow(m, -1, 1 << B)) % (1 << B)
    t = [0] * 16
    for i in range(9):
        for j in range(16):
            s = t[j] + sum(ak[i] * bk[j] for ak, bk in zip(a, b))
            assert s <= U64, "column bound"
            t[j] = s
        d = (((t[0] & U32) * ninv) & U32) & MASK
        t = [t[j] + d * pl[j] for j in range(16)]
        assert max(t) <= U64, "column bound"
        t = [(t[1] + (t[0] >> B)) & U64] + t[2:] + [0]
    h = [t[j] >> B if j < 8 else 0 for j in range(16)]
    x = [((t[j] & MASK if j < 8 else t[j]) + (h[j - 1] if j else 0)) & U64 for j in range(16)]
    h2 = [(x[j] >> B) & U32 if j < 8 else 0 for j in range(16)]
    return [(((x[j] & U32) & MASK if j < 8 else x[j] & U32) + (h2[j - 1] if j else 0)) & U32 for j in range(16)]


def mont_int(pairs, m=Q):
    """(sum a b + d m) / 2^261 with d the digit-by-digit Montgomery quotient: the integer that
    f29_mont and RowF::mont both return (a, b integers, the limb sums of the operands)"""
    t = sum(a * b for a, b in pairs)
    d = (-t * (_QINV if m == Q else pow(m, -1, R261))) % R261
    return (t + d * m) >> (9 * B)


# ---------------------------------------------------------------------------
# Q29 (one lane: normalized results)
# ---------------------------------------------------------------------------
def f29_norm(a):
    a = list(a)
    for i in range(8):
        a[i + 1] = (a[i + 1] + (a[i] >> B)) & U32
        a[i] &= MASK
    return a


def q_add(a, b):
    return f29_norm([(x + y) & U32 for x, y in zip(a, b)])


def q_sub(k, a, b):
    kb = borrowed(k)
    return f29_norm([(x + c - y) & U32 for x, c, y in zip(a, kb, b)])


def q_is_zero(k, a):
    return any(list(a) == kp_limbs(j) for j in range(k))


# ---------------------------------------------------------------------------
# the precondition of RowF::sub<K>
# ---------------------------------------------------------------------------
def sub_threshold(k, m=Q, lo=KP_LO):
    """The smallest D such that every a + K M - b >= D over lazy rows a, b comes out of sub<K> with
    its unsigned limb sum equal to the integer.

    Lane 7 of a + row_kp - b is s7 + 2^31 - 4 (s7 = a7 + (K M)7 - b7) and passes floor(.. / 2^29) =
    4 + floor((s7 - 4) / 2^29) to lane 8, which holds a8 + (K M)8 - 4 - b8 mod 2^32: the top lane
    ends at d8 + floor((s7 - 4) / 2^29) with d8 = a8 + (K M)8 - b8, and wraps below zero exactly
    when 2^29 d8 + s7 <= 3.  The integer is D = 2^232 d8 + 2^203 s7 + S', S' the part of lanes
    0..6, at most sum_{j<7} (LAZY - 1 + (K M)j) 2^(29 j): the largest D that wraps is 3 2^203 +
    max S', the threshold one more."""
    kp = kp_limbs(k, m)
    smax = sum((LAZY - 1 + kp[j]) << (B * j) for j in range(7))
    return ((lo - 1) << (B * 7)) + smax + 1


def sub_edge_case(k, at_threshold):
    """lazy rows (a, b) in sub_threshold's extreme configuration: a + K p - b is the threshold
    itself (exact), or one below it (the largest difference that wraps)"""
    kp = kp_limbs(k)
    a = [LAZY - 1] * 7 + [0, 0]
    b = ([MASK] * 7 if at_threshold else [0] * 7) + [kp[7] - (4 if at_threshold else 3), kp[8]]
    assert 0 <= b[7] < LAZY
    assert value(a) + k * Q - value(b) == sub_threshold(k) - (0 if at_threshold else 1)
    return row(a), row(b)


SUB_SAFE = 1 << 206   # above sub_threshold(K) for every K: 3 2^203 + (< 2^203 (1 + 2^-22)) + (< 2^203)


# ---------------------------------------------------------------------------
# the point formulas on integers (both policies return these integers)
# ---------------------------------------------------------------------------
def _mul(a, b):
    return mont_int([(a, b)])


def quad_dbl_int(p):
    X, Y, ZZ, ZZZ = p
    U = 2 * Y
    V, X2 = _mul(U, U), _mul(X, X)
    M = 3 * X2
    W, S, ZZ3, M2 = _mul(U, V), _mul(X, V), _mul(ZZ, V), _mul(M, M)
    X3 = M2 + 4 * Q - 2 * S
    t0, t1, t2 = _mul(M, S + 6 * Q - X3), _mul(W, Y), _mul(W, ZZZ)
    return (X3, t0 + 2 * Q - t1, ZZ3, t2)


def quad_add_int(p, o, trace=None):
    """trace: a dict that receives P and R (the values is_zero<4> sees)"""
    U1, U2, S1, S2 = _mul(p[0], o[2]), _mul(o[0], p[2]), _mul(p[1], o[3]), _mul(o[1], p[3])
    P, R = U2 + 2 * Q - U1, S2 + 2 * Q - S1
    if trace is not None:
        trace.update(P=P, R=R)
    PP, R2, Z12, ZZZ12 = _mul(P, P), _mul(R, R), _mul(p[2], o[2]), _mul(p[3], o[3])
    PPP, Qv, ZZ3 = _mul(P, PP), _mul(U1, PP), _mul(Z12, PP)
    X3 = (R2 + 2 * Q - PPP) + 4 * Q - 2 * Qv
    QX = Qv + 8 * Q - X3
    t0, t1, t2 = _mul(R, QX), _mul(S1, PPP), _mul(ZZZ12, PPP)
    return (X3, t0 + 2 * Q - t1, ZZ3, t2)


def xyzz_affine(p):
    """(X, Y, ZZ, ZZZ) in the Montgomery domain (any multiples of p) -> the affine point or None"""
    X, Y, ZZ, ZZZ = (v % Q for v in p)
    if ZZ == 0:
        return None
    # the factors 2^261 cancel: X/ZZ and Y/ZZZ are ratios of two Montgomery forms
    return (X * pow(ZZ, -1, Q) % Q, Y * pow(ZZZ, -1, Q) % Q)


def xyzz_mont(pt, z):
    """affine pt with the given z -> (x z^2, y z^3, z^2, z^3), canonical, Montgomery domain"""
    x, y = pt
    zz, zzz = z * z % Q, z * z * z % Q
    return tuple(v * R261 % Q for v in (x * zz, y * zzz, zz, zzz))


# ---------------------------------------------------------------------------
# interval walk: every value as [lo, hi) over the integers
# ---------------------------------------------------------------------------
IN_RANGE = {"X": 8, "Y": 4, "ZZ": 2, "ZZZ": 2}   # documented coordinate ranges, in multiples of p
SITE_K = {"dbl.X3": 4, "dbl.S-X3": 6, "dbl.Y3": 2, "add.P": 2, "add.R": 2, "add.R2-PPP": 2, "add.X3": 4,
          "add.Q-X3": 8, "add.Y3": 2, "glv.-Y": 4}


class Walk:
    """Interval arithmetic over the formulas; records the margin of every sub<K> site (the least
    a + K p - b minus sub_threshold(K)) and the largest product column."""

    def __init__(self, site_k=None, lo=KP_LO, hi=KP_HI):
        self.k = dict(SITE_K if site_k is None else site_k)
        self.lo, self.hi = lo, hi
        self.margin = {}
        self.worst = {}   # site -> (K, the least minuend, the largest subtrahend)
        self.column = 0

    @staticmethod
    def top(iv):
        return max(LAZY - 1, (iv[1] - 1) >> (8 * B))   # the largest limb of a lazy value below hi

    def mul(self, a, b):
        # a column of RowF::mont<1> / f29_mont<1>: nine operand products, nine reduction products
        # (digit < 2^29 times a limb of p), the carry of the column below (< 2^35)
        col = 9 * self.top(a) * self.top(b) + 9 * MASK * MASK + (1 << 35)
        self.column = max(self.column, col)
        assert col < 1 << 64, "column bound"
        assert a[1] - 1 < R261 and b[1] - 1 < R261, "top limb"
        return (0, Q + ((a[1] - 1) * (b[1] - 1) >> (9 * B)) + 1)

    def add(self, a, b):
        return (a[0] + b[0], a[1] + b[1] - 1)

    def dbl(self, a):
        return self.add(a, a)

    def sub(self, site, a, b):
        k = self.k[site]
        least = a[0] + k * Q - (b[1] - 1)
        m = least - sub_threshold(k, Q, self.lo)
        if m <= self.margin.get(site, m):
            self.margin[site], self.worst[site] = m, (k, a[0], b[1] - 1)
        assert m >= 0, f"{site}: sub<{k}> can meet a difference of {least / Q:.4f} p, below its precondition"
        # the bias keeps lanes 0..7 inside [0, 2^32) for any lazy operands
        assert self.hi - self.lo - (LAZY - 1) >= 0 and (LAZY - 1) + MASK + self.hi <= U32, "row_kp bias"
        return (least, a[1] + k * Q - b[0])

    def quad_dbl(self, p):
        X, Y, ZZ, ZZZ = p
        U = self.dbl(Y)
        V, X2 = self.mul(U, U), self.mul(X, X)
        M = self.add(self.dbl(X2), X2)
        W, S, ZZ3, M2 = self.mul(U, V), self.mul(X, V), self.mul(ZZ, V), self.mul(M, M)
        X3 = self.sub("dbl.X3", M2, self.dbl(S))
        t0, t1, t2 = self.mul(M, self.sub("dbl.S-X3", S, X3)), self.mul(W, Y), self.mul(W, ZZZ)
        return (X3, self.sub("dbl.Y3", t0, t1), ZZ3, t2)

    def quad_add(self, p, o):
        U1, U2, S1, S2 = self.mul(p[0], o[2]), self.mul(o[0], p[2]), self.mul(p[1], o[3]), self.mul(o[1], p[3])
        P, R = self.sub("add.P", U2, U1), self.sub("add.R", S2, S1)
        PP, R2, Z12, ZZZ12 = self.mul(P, P), self.mul(R, R), self.mul(p[2], o[2]), self.mul(p[3], o[3])
        PPP, Qv, ZZ3 = self.mul(P, PP), self.mul(U1, PP), self.mul(Z12, PP)
        X3 = self.sub("add.X3", self.sub("add.R2-PPP", R2, PPP), self.dbl(Qv))
        QX = self.sub("add.Q-X3", Qv, X3)
        t0, t1, t2 = self.mul(R, QX), self.mul(S1, PPP), self.mul(ZZZ12, PPP)
        return (X3, self.sub("add.Y3", t0, t1), ZZ3, t2)

    def neg_y(self, y):
        return self.sub("glv.-Y", (0, 1), y)


def in_point(rng=None):
    rng = IN_RANGE if rng is None else rng
    return tuple((0, rng[c] * Q) for c in ("X", "Y", "ZZ", "ZZZ"))


def inside(p, rng=None):
    rng = IN_RANGE if rng is None else rng
    return all(iv[1] - 1 < rng[c] * Q for iv, c in zip(p, ("X", "Y", "ZZ", "ZZZ")))


def walk(site_k=None, rng=None, lo=KP_LO, hi=KP_HI):
    """quad_dbl and quad_add from the documented input ranges, then the negation of glv_row_mul on
    what it really negates: the Y of a table entry, which is the canonical input (< p) or an output
    of quad_dbl / quad_add, and never 0 as an integer (Y = 0 mod p is a point of order 2, and the
    chains run on points of prime order).  -> the Walk, the two output points, the negated Y."""
    w = Walk(site_k, lo, hi)
    p = in_point(rng)
    d, a = w.quad_dbl(p), w.quad_add(p, p)
    y_hi = max(d[1][1], a[1][1], Q)
    ny = w.neg_y((1, y_hi))
    return w, d, a, ny
