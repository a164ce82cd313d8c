"""Synthetic circuits for the witness-program tests (tests/test_wprog.py, tests/test_gpu_wprog_ops.py):
the opcodes, Poseidon widths, live-S-box bitmaps and linear-combination shapes of csrc/witness.hip
that the five reference circuits, fed honest-client inputs, never execute.

A system is ``(Builder, [input dicts])``, built with ``zkfl.r1cs.Builder``.  Where the Builder's public
methods cannot express a shape (an op without its asserts, a combination whose coefficients vanish,
a Poseidon op with a hand-chosen live set) the op is appended to ``b.ops`` directly, its wires taken
from ``b._new_wires``: oracle/witness.py and zkfl/wprog.py both read ``b.ops``, so both follow.  Such
ops add no constraint, so these systems are witness programs, not provable circuits -- except
``e2e``, which uses the public methods only.

``system(name)`` builds a system once per process, ``reference(name)`` evaluates it with the oracle
once (``check=False`` for the ``fail_*`` systems, whose inputs violate an assert); both are shared by
the CPU and the GPU tests and must be left unchanged.
"""
import random
import re
import types
from functools import lru_cache

from oracle import witness as ow
from zkfl.field import POSEIDON_RF, POSEIDON_RP, R
from zkfl.r1cs import Builder, add, add_const, const, lc_sum, scale

HALF = (R + 1) // 2                     # 2^-1
POS_WIDTHS = tuple(range(2, 18))
CONST_LANE_WIDTHS = (6, 9, 13, 17)      # one width per pos_rounds<2..5>
BITS_WIDTHS = (1, 2, 31, 32, 33, 63, 64, 65, 253, 254)

NAMES = ("inv", "bits", "lc_mul") + tuple(f"pos_t{t}" for t in POS_WIDTHS) + ("pos_sparse", "mixed_level", "e2e")
FAIL_NAMES = ("fail_bits3", "fail_is_zero", "fail_batch")


# -- ops the Builder's methods do not emit on their own ---------------------------------------------
def raw_lc(b, lc) -> dict:
    w = b._new_wires(1)
    b.ops.append(("lc", w, dict(lc)))
    return {w: 1}


def raw_inv(b, lc) -> dict:
    w = b._new_wires(1)
    b.ops.append(("inv", w, dict(lc)))
    return {w: 1}


def raw_bits(b, lc, n) -> list:
    w0 = b._new_wires(n)
    b.ops.append(("bits", w0, n, dict(lc)))
    return [{w0 + i: 1} for i in range(n)]


def raw_pos(b, ins, live) -> list:
    """One permutation of width len(ins) + 1 writing (x^2, x^4, x^5) of the S-boxes `live` only."""
    t = len(ins) + 1
    assert list(live) == sorted(set(live)) and live[-1] < n_sbox(t)
    w0 = b._new_wires(3 * len(live))
    b.ops.append(("pos", w0, t, [dict(a) for a in ins], types.SimpleNamespace(live=list(live))))
    return [{w0 + i: 1} for i in range(3 * len(live))]


def n_sbox(t: int) -> int:
    return POSEIDON_RF * t + POSEIDON_RP[t - 2]


def _coef(rng) -> int:
    return rng.choice((1, 2, R - 1, rng.randrange(R)))


# -- the systems ---------------------------------------------------------------------------------
def _inv():
    """K_INV: is_zero gates and bare inverses of 0, of a sum that is 0 only after reduction, of
    (r-1) x, of 1, r-1, 2, 2^-1 and a random value; inverse of inverse; inv -> mul -> inv."""
    rng = random.Random(2201)
    b = Builder("inv")
    out = b.output("out")
    z, x, y = b.input("z"), b.input("x"), b.input("y")
    v = b.input("v", (5,))
    operands = [z, add(x, y), scale(x, R - 1)] + v
    res = []
    for a in operands:
        res.append(b.is_zero(a))
        res.append(raw_inv(b, a))
    for a in [x] + v:                                  # the inverse of an inverse returns the input
        back = raw_inv(b, raw_inv(b, a))
        b.assert_eq(back, a)
        res.append(back)
    i1 = raw_inv(b, add_const(x, 1))                   # two levels: inv -> mul -> inv
    m = b.mul(i1, add(x, v[4]))
    res += [i1, m, raw_inv(b, m), b.is_zero(m)]
    b.bind_output(out, lc_sum(res))
    inputs = []
    for _ in range(2):
        xv = rng.randrange(2, R - 1)
        inputs.append({"z": 0, "x": xv, "y": R - xv, "v": [1, R - 1, 2, HALF, rng.randrange(1, R)]})
    return b, inputs


def _bits():
    """K_BITS: Num2Bits at the widths around the 32-bit word boundaries and at the format's maximum,
    on 0, 1, 2^n - 1, random values and r - 1; bare decompositions of sums that wrap past r."""
    rng = random.Random(2202)
    b = Builder("bits")
    out = b.output("out")
    x = b.input("x", (len(BITS_WIDTHS),))
    p, q = b.input("p"), b.input("q")
    top = []
    for a, n in zip(x, BITS_WIDTHS):
        top.append(b.num2bits(a, n)[-1])
    for n in (254, 7):
        top += raw_bits(b, add(p, q), n)
    b.bind_output(out, lc_sum(top))
    inputs = [{"x": [0] * len(BITS_WIDTHS), "p": R - 1, "q": R - 1},
              {"x": [1] * len(BITS_WIDTHS), "p": R - 5, "q": 9},
              {"x": [(1 << n) - 1 for n in BITS_WIDTHS], "p": HALF, "q": HALF + 100},   # 2^254 - 1 wraps past r
              {"x": [rng.randrange(1 << n) for n in BITS_WIDTHS], "p": rng.randrange(R), "q": R - 1},
              {"x": [rng.randrange(1 << n) for n in BITS_WIDTHS[:-1]] + [R - 1], "p": 1, "q": R - 1}]
    return b, inputs


def _lc_mul():
    """lc_eval shapes: no terms, 1..5 and 300 terms over inputs r - 1, coefficients 1 / 2 / r - 1 /
    random, the constant wire alone, sums that are 0 only after reduction (into an assert and into a
    product), (r-1)(r-1), 0 * x, and 40 dependent squarings (40 levels of one op)."""
    rng = random.Random(2203)
    b = Builder("lc_mul")
    out = b.output("out")
    a = b.input("a", (300,))
    ng = b.input("ng", (4,))               # ng[i] = r - a[i]
    zero = b.input("zero")
    wa = [next(iter(t)) for t in a]
    res = []
    for lc in ({}, {wa[0]: 0, wa[1]: R, 0: 0}):                    # every coefficient 0 mod r
        res.append(raw_lc(b, lc))
    for c in (1, 2, R - 1, rng.randrange(R)):                      # one term, each kind of coefficient
        res.append(raw_lc(b, {wa[3]: c}))
    for n in (2, 3, 4, 5, 300):
        res.append(raw_lc(b, {w: _coef(rng) for w in rng.sample(wa, n)}))
    res.append(raw_lc(b, {w: R - 1 for w in wa}))                  # 300 x (r-1)(r-1)
    for c in (1, R - 1, rng.randrange(R)):                         # the constant wire alone
        res.append(raw_lc(b, {0: c}))
    nil = add(a[0], ng[0])                                         # nonzero parts, zero sum
    res.append(raw_lc(b, nil))
    b.assert_eq(nil, {})
    b.assert_eq(add(scale(a[1], R - 1), scale(ng[1], R - 1)), {})
    b.assert_mul(add(a[2], ng[2]), a[3], {})
    res.append(b.mul(a[0], a[1]))                                  # (r-1)(r-1) on the first input set
    res.append(b.mul(zero, a[1]))                                  # 0 * x
    res.append(b.mul(add(a[3], ng[3]), a[1]))                      # (0 after reduction) * x
    s = add_const(a[2], 3)
    for _ in range(40):
        s = b.mul(s, s)
    res.append(s)
    b.bind_output(out, lc_sum(res))
    inputs = []
    for vals in ([R - 1] * 300, [rng.randrange(R) for _ in range(300)]):
        inputs.append({"a": vals, "ng": [(R - v) % R for v in vals[:4]], "zero": 0})
    return b, inputs


def _pos_t(t):
    """64 // t + 1 permutations of width t in one level (with 2 witnesses the last wave is partial
    and one wave's jobs straddle the witnesses).  The inputs come in three groups, per witness one
    all 0, one all r - 1, one random; permutations 0..2 read a group as bare wires, the others mix
    bare wires with multi-term combinations.  For the widths of CONST_LANE_WIDTHS a second level
    holds one permutation with a constant first input and one with a constant last input."""
    rng = random.Random(2300 + t)
    b = Builder(f"pos_t{t}")
    out = b.output("out")
    m = t - 1
    x = b.input("x", (3, m))
    hs = []
    for k in range(64 // t + 1):
        g, g2 = x[k % 3], x[(k + 1) % 3]
        if k < 3:
            ins = list(g)
        else:
            ins = [g[i] if (i + k) % 2 else add_const(add(g[i], scale(g2[(i + 1) % m], _coef(rng))), k)
                   for i in range(m)]
        hs.append(b.poseidon(ins))
    if t in CONST_LANE_WIDTHS:
        mix = [add(x[2][i], scale(x[0][(i + 1) % m], 3)) if i % 2 else x[2][i] for i in range(m)]
        hs.append(b.poseidon([const(5), hs[0]] + mix[2:]))
        hs.append(b.poseidon([hs[1]] + mix[1:m - 1] + [const(7)]))
    b.bind_output(out, lc_sum(hs))             # the final state, not only the trace
    rnd = lambda: [rng.randrange(R) for _ in range(m)]  # noqa: E731
    inputs = [{"x": [[0] * m, [R - 1] * m, rnd()]}, {"x": [rnd(), [0] * m, [R - 1] * m]}]
    return b, inputs


SPARSE_17 = (0, 31, 32, 33, 63, 64, 127, 128, 191, 192, 203)     # every bitmap word, both ends of words
SPARSE_9 = (1, 30, 32, 64, n_sbox(9) - 1)


def _pos_sparse():
    """Live-S-box bitmaps with holes in every word, beside full templates of the same widths (one
    wave then holds ops of different templates)."""
    rng = random.Random(2204)
    b = Builder("pos_sparse")
    out = b.output("out")
    x = b.input("x", (16,))
    res = []
    mixed = [add_const(add(x[i], scale(x[(i + 5) % 16], _coef(rng))), i) if i % 3 == 0 else x[i] for i in range(16)]
    res += raw_pos(b, mixed, SPARSE_17)
    res.append(b.poseidon(x))
    res += raw_pos(b, x, SPARSE_17)
    res += raw_pos(b, mixed[:8], SPARSE_9)
    res.append(b.poseidon(mixed[8:]))
    res += raw_pos(b, x[8:], SPARSE_9)
    b.bind_output(out, lc_sum(res))
    inputs = [{"x": [0] * 16}, {"x": [R - 1] * 16}, {"x": [rng.randrange(R) for _ in range(16)]}]
    return b, inputs


def _mixed_level():
    """One level, reading only inputs, with every kind of segment: 70 LC ops (more than a wave), 3 MUL,
    2 INV, 2 BITS and Poseidon permutations of widths 2, 9, 13 and 17, in mixed program order; a
    second level consumes every result."""
    rng = random.Random(2205)
    b = Builder("mixed_level")
    out = b.output("out")
    x = b.input("x", (20,))

    def comb(n):
        return lc_sum(scale(x[i], _coef(rng)) for i in rng.sample(range(20), n))

    res = [b.poseidon(x[:16])]
    res += [raw_lc(b, add_const(comb(1 + k % 4), k)) for k in range(35)]
    res.append(b.mul(comb(2), comb(3)))
    res.append(b.poseidon([comb(2) for _ in range(8)]))
    res.append(raw_inv(b, comb(2)))
    res += raw_bits(b, x[0], 5)
    res.append(b.mul(x[1], x[2]))
    res.append(b.poseidon([x[19]]))
    res += [raw_lc(b, comb(1 + k % 3)) for k in range(35)]
    res.append(raw_inv(b, x[3]))
    res += raw_bits(b, comb(3), 40)
    res.append(b.poseidon(x[4:16]))
    res.append(b.mul(add_const(x[4], R - 1), x[4]))
    b.bind_output(out, lc_sum(res))
    inputs = [{"x": [rng.randrange(R) for _ in range(20)]} for _ in range(3)]
    return b, inputs


def _e2e():
    """A provable circuit (public Builder methods only) with the ops the reference circuits lack:
    an IsZero gate, a 254-bit Num2Bits and a width-9 Poseidon, one bound output."""
    rng = random.Random(2206)
    b = Builder("e2e")
    out = b.output("out")
    x, y = b.input("x"), b.input("y")
    v = b.input("v", (4,))
    bits = b.num2bits(y, 254)
    h = b.poseidon([b.is_zero(x), b.is_zero(add_const(y, 1)), bits[0], bits[253]] + v)
    b.bind_output(out, h)
    inputs = [{"x": 0, "y": R - 1, "v": [rng.randrange(R) for _ in range(4)]},
              {"x": rng.randrange(1, R), "y": rng.randrange(R - 1), "v": [0, 1, R - 1, HALF]}]
    return b, inputs


def _fail_bits3():
    b = Builder("fail_bits3")
    b.num2bits(b.input("x"), 3)
    return b, [{"x": 8}]


def _fail_is_zero():
    b = Builder("fail_is_zero")
    b.assert_eq(b.is_zero(b.input("x")), const(1))
    return b, [{"x": 5}]


def _fail_batch():
    """Witness 0 holds; witness 1 fails the sum of the first Num2Bits and that of the second."""
    b = Builder("fail_batch")
    x, y = b.input("x"), b.input("y")
    b.assert_mul(x, y, scale(b.mul(x, y), 1))
    b.num2bits(x, 3)
    b.num2bits(y, 4)
    return b, [{"x": 7, "y": 15}, {"x": 9, "y": 16}]


_BUILD = {"inv": _inv, "bits": _bits, "lc_mul": _lc_mul, "pos_sparse": _pos_sparse, "mixed_level": _mixed_level,
          "e2e": _e2e, "fail_bits3": _fail_bits3, "fail_is_zero": _fail_is_zero, "fail_batch": _fail_batch}


@lru_cache(maxsize=None)
def system(name):
    """-> (Builder, [input dicts]); built once, shared, not to be modified."""
    if name.startswith("pos_t"):
        return _pos_t(int(name[5:]))
    return _BUILD[name]()


def all_systems():
    for name in NAMES + FAIL_NAMES:
        yield (name,) + system(name)


@lru_cache(maxsize=None)
def reference(name):
    """The oracle's witness (tuple of ints, wire order) of every input of a system."""
    b, inputs = system(name)
    return tuple(tuple(ow.evaluate(b, x, check=name not in FAIL_NAMES)) for x in inputs)


def failing_asserts(b, w) -> list:
    """Positions in ``b.asserts`` of the asserts the witness `w` violates."""
    bad = []
    for pos, ci in enumerate(b.asserts):
        A, B, C = b.cons[ci]
        if ow._ev(A, w) * ow._ev(B, w) % R != ow._ev(C, w):
            bad.append(pos)
    return bad


def first_failure(name):
    """(witness, position in b.asserts) of the failure the engine must report for a fail_* system:
    the lowest failing witness and its lowest failing assert.  The assert comes from the oracle's
    AssertFailed, which names the index into ``b.cons``."""
    b, inputs = system(name)
    for j, x in enumerate(inputs):
        try:
            ow.evaluate(b, x)
        except ow.AssertFailed as e:
            ci = int(re.search(r"assert constraint (\d+) failed", str(e)).group(1))
            return j, b.asserts.index(ci)
    raise AssertionError(f"{name}: every input satisfies the asserts")
