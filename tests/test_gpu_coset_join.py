"""The polynomial stage's last step, the coset transform of a, b, c and the join (zkfl_debug_coset_join:
ntt_coset_shift on the three vectors, then k_join, as the prover's abc_ntt calls them), against the
C oracle -- run on an MI355X (-m gpu).

h = a b - c on the odd coset, standard form.  The expected value is the oracle's coset transform
(cbaseline.coset_ntt, as tests/test_gpu_ntt.py takes it) of a, b and c, then A B - C mod r in Python
integers; the comparison is bit for bit.  Domains: 2^1 .. 2^10 have no column pass (at 2^1 and 2^2
the product-free span-1 step and the span-2 stages are the whole transform); 2^11 is the column
pass at k = 1 (512 columns per workgroup), 2^12 and 2^14 mid sizes of the pair schedule, 2^20 k = 10
(one column per workgroup, run once); col_max = 0 forces the large-domain schedule.  Whatever forms
h (today k_join everywhere; a forward column pass that joined was measured and not kept, DESIGN.md
§5) has to pass these cases.  Inputs: seeded random, all zero, every element r - 1, c = a o b on the
domain (the prover's case: a b - c vanishes there, not on the coset), and a single non-zero element
at index 0 and at n - 1.
"""
import functools
import random

import pytest

import ntt_vectors as nv

pytestmark = pytest.mark.gpu

R = nv.R
KINDS = ("random", "zero", "all_r_minus_1", "c_is_ab", "single_first", "single_last")
# (logn, col_max): the default schedule, and the large-domain one forced at small sizes
DOMAINS = [(1, -1), (2, -1), (3, -1), (10, -1), (11, -1), (12, -1), (14, -1), (12, 0), (14, 0)]


def _oracle(data):
    from oracle import cbaseline
    return cbaseline.coset_ntt(data, cbaseline.default_threads())


def _pack(vals):
    return b"".join(nv.le(v) for v in vals)


def _inputs(logn, kind):
    n = 1 << logn
    if kind == "random":
        return [nv.random_vec(logn, 7000 * logn + v) for v in range(3)]
    if kind == "zero":
        return [bytes(32 * n)] * 3
    if kind == "all_r_minus_1":
        return [nv.le(R - 1) * n] * 3
    if kind == "c_is_ab":
        a, b = (nv.random_vec(logn, 9000 * logn + v) for v in range(2))
        return [a, b, _pack(x * y % R for x, y in zip(nv.ints(a), nv.ints(b)))]
    at = 0 if kind == "single_first" else n - 1
    rng = random.Random(100 * logn + at % 7)
    out = []
    for _ in range(3):
        v = bytearray(32 * n)
        v[32 * at:32 * at + 32] = nv.le(rng.randrange(1, R))
        out.append(bytes(v))
    return out


def _want(vecs):
    A, B, C = (nv.ints(_oracle(v)) for v in vecs)
    return _pack((x * y - z) % R for x, y, z in zip(A, B, C))


@functools.lru_cache(maxsize=None)
def _case(logn, kind):
    """The three input vectors (one buffer) and the expected h, computed once per session."""
    vecs = _inputs(logn, kind)
    return b"".join(vecs), _want(vecs)


def _check(got, want, what):
    if got == want:
        return
    assert len(got) == len(want), what
    bad = [i // 32 for i in range(0, len(want), 32) if got[i:i + 32] != want[i:i + 32]]
    pytest.fail(f"{what}: {len(bad)} of {len(want) // 32} elements of h differ from the oracle, the first at index {bad[0]}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("logn,col_max", DOMAINS)
def test_coset_join_matches_oracle(gpu_ctx, logn, col_max, kind):
    abc, want = _case(logn, kind)
    _check(gpu_ctx.debug_coset_join(abc, logn, col_max), want, f"2^{logn} col_max {col_max} {kind}")


def test_coset_join_2_20(gpu_ctx):
    """k = 10: one column per workgroup of the column passes."""
    vecs = _inputs(20, "random")
    _check(gpu_ctx.debug_coset_join(b"".join(vecs), 20), _want(vecs), "2^20 random")


def test_coset_join_reads_c(gpu_ctx):
    """One element of c changed changes h (a kernel that ignored c could not pass), and the changed
    h is the oracle's."""
    logn = 12
    n = 1 << logn
    abc, want = _case(logn, "random")
    at = 32 * (2 * n + 1234)
    old = int.from_bytes(abc[at:at + 32], "little")
    changed = abc[:at] + nv.le((old + 1) % R) + abc[at + 32:]
    got = gpu_ctx.debug_coset_join(changed, logn)
    assert got != want
    _check(got, _want([changed[32 * n * v:32 * n * (v + 1)] for v in range(3)]), "2^12 random, one element of c changed")


def test_coset_join_argument_errors(gpu_ctx):
    import ctypes
    from zkfl import native
    L = native.lib()
    buf = bytes(3 * 8 * 32)
    out = (ctypes.c_uint8 * (8 * 32))()
    assert L.zkfl_debug_coset_join(gpu_ctx.h, buf, 0, -1, out) == -1
    assert L.zkfl_debug_coset_join(gpu_ctx.h, buf, 28, -1, out) == -1
    assert L.zkfl_debug_coset_join(gpu_ctx.h, None, 3, -1, out) == -1
    assert L.zkfl_debug_coset_join(gpu_ctx.h, buf, 3, -1, None) == -1
    assert L.zkfl_debug_coset_join(gpu_ctx.h, buf, 3, 11, out) == -1
    assert L.zkfl_debug_coset_join(None, buf, 3, -1, out) == -1
