"""The MSM stage of a small key's proof (csrc/prove.hip front_msm, the function run_front calls)
on chosen inputs, through the parity hook zkfl_debug_msm_front -- run on an MI355X (-m gpu).

Every key with a domain of at most 2^16 proves through this launch sequence and nothing else does:
msm_sort_multi (the sorts of all sets in the same four launches), k_msm_accumulate_multi (their
accumulations in one launch), B2 on G2 lane pairs from B1's sorted pairs with B1's entry count, and
msm_tails_joint (k_msm_stitch_joint, k_msm_stitch_last_joint, k_msm_wsum_joint: both curves in one
grid).  A satisfiable witness on an honest key cannot make one set empty, one tail deep beside
shallow ones, a bucket open across chunk edges in one set only, or P + P inside a G2 lane pair; these
inputs do.  joint = 0 runs the batched msm_tails (n > 1, with and without the fast reduction), the
form of the other two schedules, on the same inputs.

Bar: bit-exact.  Bases are k_i G (g1_gen_mul / g2_gen_mul), expectations (sum k_i s_i mod r) G from
Python integers by oracle/bn254.py: one oracle multiplication per result, None (infinity) when the
sum is 0.  The G1 set that plays B1 and the G2 set get different k over the same scalars, so a result
copied across curves cannot pass.  One case takes oracle-made points and bn.msm instead.

The two bucket reductions (fast = 0 / 1) give the same point by construction, so these tests check
that each is right on every input, not which of the two a flag selects.

The sizes assume MSM_SG = 8, MSM_SMALL_L = 8, MSM_STITCH_LAST = 128 (csrc/msm_api.h, csrc/msm.h)
and sort blocks of 256 bases (csrc/msm_sort.h); each is derived where it is chosen.
"""
import random
import zlib

import pytest

from oracle import bn254 as bn

pytestmark = pytest.mark.gpu

R = bn.R

CASES = ["zeros", "ones", "small", "neg", "max", "dup", "cancel", "inf_base", "binedge14", "binedge16"]


def _scal(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def _scalars(case, n, rnd):
    """n scalars of a value case (the cases of test_gpu_parity.py::test_msm_g1_edge_cases)."""
    if case == "zeros":
        return [0] * n
    if case == "ones":          # every entry in bucket 0: one run open across every chunk edge
        return [1] * n
    if case == "small":         # witness-like bits / small ints
        return [rnd.choice([0, 1, 2, 3, 100, 65535, 65536, 1 << 15, (1 << 15) + 1, (1 << 16) + 1, (1 << 17) - 1,
                            1 << 17, (1 << 17) + 1, (1 << 13) + 1, 1 << 13]) for _ in range(n)]
    if case == "neg":           # digits near the signed boundary
        return [R - rnd.randrange(1, 1 << 20) for _ in range(n)]
    if case == "max":
        return [R - 1] * n
    if case == "dup":           # one scalar for every base
        return [rnd.randrange(R)] * n
    if case == "cancel":        # pairs of equal scalars
        half = [rnd.randrange(R) for _ in range((n + 1) // 2)]
        return [half[i // 2] for i in range(n)]
    if case == "binedge14":     # 14-bit windows: bucket 2^13 - 1, the signed-digit boundary 2^13 / 2^13 + 1 and
        # the high-bin edges of the sort's 6 low bits
        edge = [1, 2, 63, 64, 65, 127, 8191, 8192, 8193, 16383, 0]
        return [sum(rnd.choice(edge) << (14 * j) for j in range(19)) % R for _ in range(n)]
    if case == "binedge16":     # 16-bit windows: bucket 2^15 - 1, 2^15 / 2^15 + 1, the edges of 8 low bits
        edge = [1, 2, 255, 256, 257, 512, 32767, 32768, 32769, 65535]
        return [sum(rnd.choice(edge) << (16 * j) for j in range(16)) % R for _ in range(n)]
    assert case in ("random", "inf_base"), case
    return [rnd.randrange(R) for _ in range(n)]


def _mults(case, n, rnd, inf_at=0):
    """The multipliers k_i of a set's bases k_i G for a value case; 0 stands for the point at infinity."""
    ks = [rnd.randrange(1, R) for _ in range(n)]
    if case == "dup":           # the same base everywhere: P + P inside a bucket
        ks = ks[:1] * n
    elif case == "cancel":      # P and -P under equal scalars: P - P inside a bucket
        ks = [ks[i // 2] if i % 2 == 0 else R - ks[i // 2] for i in range(n)]
    elif case == "inf_base":
        ks = [0 if i % 3 == inf_at else k for i, k in enumerate(ks)]
    return ks


class _Set:
    """One G1 set of a call: multipliers, scalars and (optionally) a key's index map."""

    def __init__(self, ks, ss, sidx=None, extra_start=0, extra=()):
        self.ks, self.ss, self.sidx, self.extra_start, self.extra = ks, ss, sidx, extra_start, list(extra)

    def scalar_of(self, j):
        if self.sidx is None:
            return self.ss[j]
        si = self.sidx[j]
        return self.ss[si] if si < self.extra_start else self.extra[si - self.extra_start]

    def expect(self, ks=None):
        ks = self.ks if ks is None else ks
        return sum(k * self.scalar_of(j) for j, k in enumerate(ks)) % R

    def args(self, ctx):
        bases = ctx.g1_gen_mul(_scal(self.ks))
        if self.sidx is None:
            return (bases, _scal(self.ss))
        return (bases, _scal(self.ss), self.sidx, self.extra_start, _scal(self.extra))


class _Call:
    """The inputs of one hook call as bytes and the expected points; built once, run many times."""

    def __init__(self, ctx, sets, b, k2):
        assert len(k2) == len(sets[b].ks)
        self.args = [s.args(ctx) for s in sets]
        self.b = b
        self.g2 = ctx.g2_gen_mul(_scal(k2))
        w1 = [s.expect() for s in sets]
        w2 = sets[b].expect(k2)
        self.want1 = [bn.mul(bn.G1_GEN, w) if w else None for w in w1]
        self.want2 = bn.mul(bn.G2_GEN, w2) if w2 else None

    def run(self, ctx, fast, joint):
        return ctx.msm_front(self.args, self.b, self.g2, fast=fast, joint=joint)

    def check(self, ctx, fast, joint, tag=""):
        o1, o2 = self.run(ctx, fast, joint)
        for i, (o, w) in enumerate(zip(o1, self.want1)):
            assert bn.g1_from_bytes_std(o) == w, (tag, "G1 set", i, "fast", fast, "joint", joint)
        assert bn.g2_from_bytes_std(o2) == self.want2, (tag, "G2", "fast", fast, "joint", joint)
        return o1, o2


_calls = {}


def _cached(key, make):
    """One _Call per key for the whole module: joint x fast x width reuse inputs and expectations."""
    if key not in _calls:
        _calls[key] = make()
    return _calls[key]


def _value_call(ctx, mix):
    """Three sets of three different value cases, so what one blockIdx.y does differs from its
    neighbours.  A and C + H have 3000 bases: 3000 x 19 windows = 57,000 digits, 7,125 chunks of 8,
    14,250 level-1 items -> 1,782 lanes (> 128: k_msm_stitch_joint), 3,564 items -> 446 lanes (> 128: a
    second joint level), 892 items -> 112 lanes: the last-levels kernel.  B, which carries G2, has
    1500: 28,500 digits, 7,126 items -> 891 lanes, 1,782 items -> 223 lanes, 446 items -> 56 lanes: two
    joint levels as well, each with fewer lanes than its neighbours'.  Sets of few digits (zeros, ones,
    small) finish levels earlier."""
    def make():
        rnd = random.Random(zlib.crc32("/".join(mix).encode()))
        ns = (3000, 1500, 3000)
        sets = [_Set(_mults(c, n, rnd), _scalars(c, n, rnd)) for c, n in zip(mix, ns)]
        # the G2 set: the same case on its own multipliers; its infinities fall on other bases than B1's
        k2 = _mults(mix[1], ns[1], rnd, inf_at=1)
        return _Call(ctx, sets, 1, k2)
    return _cached(("value",) + tuple(mix), make)


# every case once in each of the three places (so once as B, with G2 on it)
MIXES = [tuple(CASES[(i + j) % len(CASES)] for j in range(3)) for i in range(len(CASES))]


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("joint", [0, 1])
@pytest.mark.parametrize("mix", MIXES, ids="-".join)
def test_front_value_cases(gpu_ctx, monkeypatch, mix, joint, fast):
    """Value cases per set, mixed across the sets of one call, at the small keys' 14-bit windows.
    inf_base: production compacts infinity bases away at key load; the hook hands them to the
    kernels, so this reaches the kernels' own handling of a (0, 0) base."""
    monkeypatch.setenv("ZKFL_MSM_C", "14")
    _value_call(gpu_ctx, mix).check(gpu_ctx, fast, joint, mix)


MIXES16 = [("ones", "dup", "cancel"), ("cancel", "binedge16", "ones"), ("dup", "ones", "binedge16"),
           ("binedge16", "cancel", "dup")]


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("joint", [0, 1])
@pytest.mark.parametrize("mix", MIXES16, ids="-".join)
def test_front_value_cases_width16(gpu_ctx, monkeypatch, mix, joint, fast):
    """The skewed cases again at 16-bit windows (a key of more than 2^16 bases with a small domain):
    16 windows, 2^15 buckets, the other instantiation of every reduction kernel."""
    monkeypatch.setenv("ZKFL_MSM_C", "16")
    _value_call(gpu_ctx, mix).check(gpu_ctx, fast, joint, mix)


@pytest.mark.parametrize("joint", [0, 1])
@pytest.mark.parametrize("which", ["b1_only", "b2_only"])
def test_front_inf_base_on_one_curve(gpu_ctx, monkeypatch, which, joint):
    """A base that is infinity in B1 but not in B2, and the reverse: B2 accumulates from B1's sorted
    pairs, so an entry exists on both curves and one of them adds (0, 0).  Production compacts such
    bases away at key load; the hook reaches the kernels' own handling."""
    monkeypatch.setenv("ZKFL_MSM_C", "14")

    def make():
        rnd = random.Random(zlib.crc32(which.encode()))
        n = 1500
        sets = [_Set(_mults("random", n, rnd), _scalars(c, n, rnd)) for c in ("random", "small", "random")]
        k2 = _mults("random", n, rnd)
        hit = sets[1].ks if which == "b2_only" else k2   # the curve that keeps its bases
        gone = k2 if which == "b2_only" else sets[1].ks
        for i in range(0, n, 3):
            gone[i] = 0
        assert all(hit) and not all(gone)
        return _Call(gpu_ctx, sets, 1, k2)
    _cached(("inf1", which), make).check(gpu_ctx, 1, joint, which)


# Ragged and empty sets.  A sort block is 256 bases: 255 / 256 / 257 are one block less one, one
# block, two blocks, and 3000 is 12 blocks, so the sort grid (x = the largest job) is wider than the
# other jobs.  40 bases x 19 = 760 digits = 95 chunks = 190 items -> 24 lanes: that tail is in its
# last levels while the 3000-base one (1,782 lanes) still runs joint levels; 1 base has <= 19 digits, 0
# bases none.  With B the largest set G2 is the deep tail beside shallow G1 ones, with B the smallest
# it is the reverse.
TRIPLES = [(1, 257, 3000), (3000, 40, 255), (256, 3000, 0), (0, 1, 0), (40, 3000, 40)]


def _ragged_call(ctx, ns, b):
    def make():
        rnd = random.Random(zlib.crc32(repr((ns, b)).encode()))
        sets = [_Set(_mults("random", n, rnd), _scalars("random", n, rnd)) for n in ns]
        return _Call(ctx, sets, b, _mults("random", ns[b], rnd))
    return _cached(("ragged", ns, b), make)


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("joint", [0, 1])
@pytest.mark.parametrize("b_is", ["largest", "smallest"])
@pytest.mark.parametrize("ns", TRIPLES, ids=lambda t: "x".join(map(str, t)))
def test_front_ragged_and_empty_sets(gpu_ctx, monkeypatch, ns, b_is, joint, fast):
    monkeypatch.setenv("ZKFL_MSM_C", "14")
    b = ns.index(max(ns)) if b_is == "largest" else ns.index(min(ns))
    call = _ragged_call(gpu_ctx, ns, b)
    if ns[b] == 0:  # an empty B set (n_b = 0): infinity on both curves
        assert call.want1[b] is None and call.want2 is None
    call.check(gpu_ctx, fast, joint, (ns, b))


@pytest.mark.parametrize("joint", [0, 1])
@pytest.mark.parametrize("ns,b", [((300, 3000, 40, 1000), 1), ((255, 40, 3000, 257), 3), ((3000,), 0), ((1,), 0)])
def test_front_four_sets_and_one(gpu_ctx, monkeypatch, ns, b, joint):
    """n1 = 4 (the parts mode of a small key: A, B1, C, H apart, MSM_TAIL_MAX tails in one batch)
    and n1 = 1."""
    monkeypatch.setenv("ZKFL_MSM_C", "14")
    _ragged_call(gpu_ctx, ns, b).check(gpu_ctx, 1, joint, (ns, b))


@pytest.mark.parametrize("deep", [0, 1])
def test_front_one_deep_bucket_beside_shallow(gpu_ctx, monkeypatch, deep):
    """60,000 bases with scalar 1 in one set (one bucket: 7,500 chunks of 8, 15,000 items -> 1,875
    lanes, 3,750 -> 469, 938 -> 118: three joint levels by its own count, more by the host's bound of
    60,000 x 19 digits), 40 bases in the others, joint tails.  deep = 1: the deep set is B, so G2 is
    the deep tail; deep = 0: it is A and G2 rides on a 40-base set."""
    monkeypatch.setenv("ZKFL_MSM_C", "14")
    rnd = random.Random(77 + deep)
    ns = [40, 40, 40]
    ns[deep] = 60000
    sets = [_Set(_mults("random", n, rnd), [1] * n if n > 40 else _scalars("random", n, rnd)) for n in ns]
    _Call(gpu_ctx, sets, 1, _mults("random", ns[1], rnd)).check(gpu_ctx, 1, 1, deep)


@pytest.mark.parametrize("joint", [0, 1])
@pytest.mark.parametrize("target", [1, 64])
def test_front_forced_chunk_lengths(gpu_ctx, monkeypatch, target, joint):
    """ZKFL_MSM_TARGET forces the resident-lane target, so the chunk length is ceil(nnz / target)
    per set, at least MSM_SMALL_L = 8 (csrc/msm_api.h msm_chunk_len).  40 random scalars have ~760
    digits, 3000 ones 3000, 255 small scalars at most 2 each: at target 1 every set is one chunk of
    ~760 / 3000 / <= 510 entries, at target 64 the chunks hold 12 / 47 / 8 -- L differs per blockIdx.y
    inside one accumulation launch and one stitching launch, with chunk edges anywhere in a bucket."""
    monkeypatch.setenv("ZKFL_MSM_C", "14")
    monkeypatch.setenv("ZKFL_MSM_TARGET", str(target))

    def make():
        rnd = random.Random(zlib.crc32(b"chunks"))
        ns, cases = (40, 3000, 255), ("random", "ones", "small")
        sets = [_Set(_mults("random", n, rnd), _scalars(c, n, rnd)) for c, n in zip(cases, ns)]
        return _Call(gpu_ctx, sets, 1, _mults("random", ns[1], rnd))
    _cached("chunks", make).check(gpu_ctx, 1, joint, target)


def _mapped_call(ctx):
    """Every set with an index map, as every production key has: shuffled entries, many bases on
    one scalar, bases on the extra vector; the third set has all its bases there, as H's are."""
    def make():
        rnd = random.Random(zlib.crc32(b"sidx"))
        # A: 3000 bases over 500 scalars (about 6 bases per scalar) and 4 extra slots right behind
        # them (extra_start = the scalar count, as a key's is its wire count)
        ss = _scalars("random", 500, rnd)
        sidx = [rnd.randrange(500) for _ in range(2990)] + [500 + rnd.randrange(4) for _ in range(10)]
        rnd.shuffle(sidx)
        a = _Set(_mults("random", 3000, rnd), ss, sidx, 500, _scalars("random", 4, rnd))
        # B: 1500 bases, a shuffled one-to-one map over 1490 scalars of small values and ten bases on
        # extra slots; extra_start above the scalar count (the entries between are never addressed)
        sidx = list(range(1490)) + [4096 + (i % 3) for i in range(10)]
        rnd.shuffle(sidx)
        b = _Set(_mults("random", 1500, rnd), _scalars("small", 1490, rnd), sidx, 4096, [1, R - 1, 12345])
        # C + H-like: every base on the extra vector, in shuffled order; the scalar vector unused
        sidx = [7 + i for i in range(1000)]
        rnd.shuffle(sidx)
        c = _Set(_mults("random", 1000, rnd), _scalars("random", 3, rnd), sidx, 7, _scalars("random", 1000, rnd))
        return _Call(ctx, [a, b, c], 1, _mults("random", 1500, rnd))
    return _cached("mapped", make)


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("joint", [0, 1])
def test_front_index_maps(gpu_ctx, monkeypatch, joint, fast):
    """The sort's sidx / extra indirection (csrc/msm_sort.hip msm_for_digits), which the single-MSM
    primitives never pass: the expectation follows the map."""
    monkeypatch.setenv("ZKFL_MSM_C", "14")
    _mapped_call(gpu_ctx).check(gpu_ctx, fast, joint, "mapped")


def test_front_oracle_points(gpu_ctx, monkeypatch):
    """40 oracle-made points per set against the oracle's own MSM, so that not everything rests on
    the generator-multiple kernels: points, encodings and sums all come from oracle/bn254.py."""
    monkeypatch.setenv("ZKFL_MSM_C", "14")
    rnd = random.Random(11)
    pts = [[bn.mul(bn.G1_GEN, rnd.randrange(R)) for _ in range(40)] for _ in range(3)]
    pts2 = [bn.mul(bn.G2_GEN, rnd.randrange(R)) for _ in range(40)]
    ss = [[rnd.randrange(R) for _ in range(40)] for _ in range(3)]
    sets = [(b"".join(bn.g1_to_bytes_mont(p) for p in ps), _scal(s)) for ps, s in zip(pts, ss)]
    g2 = b"".join(bn.g2_to_bytes_mont(p) for p in pts2)
    want1, want2 = [bn.msm(p, s) for p, s in zip(pts, ss)], bn.msm(pts2, ss[1])
    for joint in (1, 0):
        o1, o2 = gpu_ctx.msm_front(sets, 1, g2, fast=True, joint=joint)
        assert [bn.g1_from_bytes_std(o) for o in o1] == want1, joint
        assert bn.g2_from_bytes_std(o2) == want2, joint


def test_front_repeat_on_one_context(gpu_ctx, monkeypatch):
    """The same call twice with a different one in between gives equal bytes: nothing (live
    flags, entry counts, items, buckets) survives from one call to the next."""
    monkeypatch.setenv("ZKFL_MSM_C", "14")
    x = _value_call(gpu_ctx, ("cancel", "dup", "ones"))
    y = _ragged_call(gpu_ctx, (256, 3000, 0), 2)
    first = x.check(gpu_ctx, 1, 1, "first")
    y.check(gpu_ctx, 1, 1, "between")
    assert x.check(gpu_ctx, 1, 1, "again") == first
    assert y.run(gpu_ctx, 0, 0) == y.run(gpu_ctx, 1, 1)


def test_front_argument_errors(gpu_ctx):
    """Bad inputs are refused on the host (ZKFL_E_ARG), before any device call: a hook that let an
    index map or a short vector read out of bounds would be a fault generator, not a test."""
    from zkfl import native
    g1, g2 = gpu_ctx.g1_gen_mul(_scal([1, 2, 3])), gpu_ctx.g2_gen_mul(_scal([1, 2, 3]))
    ok = (g1, _scal([5, 6, 7]))

    def refused(sets, b=0, bases_g2=g2, match=None):
        with pytest.raises(native.ZkflError, match=match) as e:
            gpu_ctx.msm_front(sets, b, bases_g2)
        assert e.value.code == -1

    refused([(g1, _scal([5, R, 7]))], match="scalar 1 is not < r")
    refused([ok, (g1, _scal([5, 6]))], match="set 1: fewer scalars than bases")
    refused([(g1, _scal([5, 6]), [0, 1, 2], 2, _scal([]))], match="sidx 2 is out of range")       # past extra
    refused([(g1, _scal([5, 6]), [0, 1, 2], 3, _scal([9]))], match="sidx 2 is out of range")      # past scalars
    refused([(g1, _scal([5, 6]), [0, 1, 3], 2, _scal([9]))], match="sidx 2 is out of range")
    refused([(g1, _scal([5, 6]), [0, 1, 2], 2, _scal([R]))], match="extra scalar 0 is not < r")
    refused([ok], bases_g2=g2[:256], match="one base per base of set b")
    refused([ok], b=1)
    refused([ok] * 5)
    # and the same shapes, in range, are served
    o1, o2 = gpu_ctx.msm_front([(g1, _scal([5, 6]), [0, 1, 2], 2, _scal([9]))], 0, g2)
    assert bn.g1_from_bytes_std(o1[0]) == bn.mul(bn.G1_GEN, 5 + 12 + 27)
    assert bn.g2_from_bytes_std(o2) == bn.mul(bn.G2_GEN, 5 + 12 + 27)
