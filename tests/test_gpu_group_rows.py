"""Grouped ABC: one QAP row evaluated per class of equal mapped rows (csrc/groups.h)
-- MI355X (-m gpu).

The partition is a speed hint: a | b | c on the domain (zkfl_debug_abc, which runs the ABC stage on
a slot as a proof does) must equal, word for word, what Python computes from the builder's
constraints and the oracle's witness, for any partition and any witness; and proofs stay the C
oracle's bytes.

Circuits: poseidon_hash2 and sgd_verified(8, 4, 3, 1000).  Counted on the CPU for the latter with
the partition learned from client 1 before the key splits groups by query: 6,132 classes of
non-empty rows and 52,188 of 258,327 terms; client 2 misses on 3 wires and dirties 14 constraints.
The key's split only makes the partition finer, so it reports at least those classes and terms, and
the grouped ABC is kept only up to K / 2 terms.  No wire of the circuit but wire 0 sits in more than
256 constraints (the next have 132), so the over-the-cap case lowers the cap (ZKFL_GROUP_ROWS_CAP).
Both circuits are small keys, which keep the plain ABC by default (config 5 lost 4 to 6 % to the
grouped form's extra launches), so the grouped ABC is tested with ZKFL_SMALL_LOGN=0 and the default
is tested to build no row classes and to prove the same bytes.
"""
import random

import pytest

pytestmark = pytest.mark.gpu

KNOBS = ("ZKFL_GRAPH", "ZKFL_STAGGER", "ZKFL_LOWLAT", "ZKFL_FAST_WSUM", "ZKFL_SMALL_LOGN", "ZKFL_AB_SHARED",
         "ZKFL_GROUPS", "ZKFL_GROUP_MIN_BATCH", "ZKFL_MSM_C", "ZKFL_GROUP_ROWS", "ZKFL_GROUP_ROWS_CAP")
TAU_SQ = 100000000
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def _le(x):
    return int(x).to_bytes(32, "little")


def _env(monkeypatch, setting, small_logn="0"):
    """Both circuits are small keys (domain <= 2^16), which keep the plain ABC by default, so the
    tests of the grouped ABC run with ZKFL_SMALL_LOGN=0 (the large-key chain) unless they say
    otherwise (small_logn=None: the default)."""
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    if small_logn is not None:
        monkeypatch.setenv("ZKFL_SMALL_LOGN", small_logn)
    for name, value in setting.items():
        monkeypatch.setenv(name, value)


def _abc_bytes(b, w, dom):
    """a | b | c on the domain from the constraints (snarkjs adds the rows n_cons + k: wire k to A for
    the public wires; the rest of the domain is padding)."""
    a, bb = [0] * dom, [0] * dom
    for j, (A, B, _c) in enumerate(b.cons):
        a[j] = sum(c * w[i] for i, c in A.items()) % R
        bb[j] = sum(c * w[i] for i, c in B.items()) % R
    for k in range(b.n_public + 1):
        a[len(b.cons) + k] = w[k] % R
    return b"".join(_le(x) for x in a + bb + [x * y % R for x, y in zip(a, bb)])


class Case:
    """A circuit, its key, witnesses, the expected a | b | c of each and (r, s) with the C oracle's
    proofs for the first two: computed once and left unchanged."""

    def __init__(self, ctx, b, inputs, seed):
        from oracle import cbaseline
        from oracle import witness as ow
        from zkfl import zkey
        self.b = b
        self.zk = zkey.groth16_setup(b, ctx, zkey.Toxic(tau=seed, alpha=seed + 1, beta=seed + 2, gamma=seed + 3,
                                                       delta=seed + 4))
        self.w = [ow.evaluate(b, i) for i in inputs]
        self.wts = [zkey.wtns_bytes(w) for w in self.w]
        self.n = len(self.w[0])
        self.dom = 1 << (len(b.cons) + b.n_public).bit_length()
        self.abc = [_abc_bytes(b, w, self.dom) for w in self.w]
        self.rs = [_le(0x1234567) + _le(0x7654321), _le(R - 1) + _le(R - 2)]
        self.proofs = [cbaseline.prove(self.zk, self.wts[i], self.rs[i]) for i in range(2)]


@pytest.fixture(scope="module")
def hash2(gpu_ctx):
    from zkfl import circuits
    ins = [{"left": 1, "right": 2}, {"left": R - 1, "right": 5}]
    return Case(gpu_ctx, circuits.build("poseidon_hash2"), ins, 0x7A1)


@pytest.fixture(scope="module")
def sgd(gpu_ctx):
    """witnesses 0, 1: clients 1 and 2; 2: client 1 with its sample rows rotated by one (the pattern
    of shared Merkle nodes breaks: many misses); 3: client 1 with the last constraint's output and
    nothing else changed (see test_only_miss_in_the_last_constraint)"""
    from zkfl import circuits, clients
    ins = [clients.Client(cid, 8, 4, 3, clients.JsLcg(12345)).training_input(8, 1000, TAU_SQ)[0] for cid in (1, 2)]
    rot = dict(ins[0])
    for k in ("features", "labels", "siblings", "pathIndices"):
        rot[k] = [ins[0][k][p] for p in (1, 2, 3, 4, 5, 6, 7, 0)]
    return Case(gpu_ctx, circuits.build("sgd_verified", 8, 4, 3, 1000), ins + [rot], 0x7B2)


def _check(key, res, want, grouped=True):
    got, miss, dirty, plain = key.debug_abc(res, grouped)
    assert len(got) == len(want)
    if got != want:
        bad = [i for i in range(len(want) // 32) if got[32 * i:32 * i + 32] != want[32 * i:32 * i + 32]]
        raise AssertionError(f"{len(bad)} of {len(want) // 32} values differ, first at {bad[:8]}")
    return miss, dirty, plain


@pytest.mark.parametrize("circuit", ["hash2", "sgd"])
@pytest.mark.parametrize("part", ["learned", "identity", "none"])
def test_partitions_that_hold(request, monkeypatch, circuit, part):
    from zkfl import native
    case = request.getfixturevalue(circuit)
    _env(monkeypatch, {})
    with native.Context(0) as ctx:
        key = native.ProvingKey(ctx, case.zk)
        assert key.domain_size == case.dom
        res = key.upload(case.wts[0])
        if part == "learned":
            key.learn_groups(res)
        elif part == "identity":
            key.set_groups(list(range(case.n)))
        else:
            key.set_groups(None)
        g = key.groups()
        print(circuit, part, {k: g[k] for k in ("rows_grouped", "row_classes", "terms", "terms_rep", "wire_list",
                                                "wires_over_cap", "rows_build_ms", "build_ms")})
        assert g["grouped"] == (part != "none")
        if part == "none":
            assert not g["rows_grouped"] and g["row_classes"] == 0 and g["terms_rep"] == g["terms"]
        else:
            assert g["rows_grouped"] == (2 * g["terms_rep"] <= g["terms"]) and g["row_classes"] > 0
        if (circuit, part) == ("sgd", "learned"):
            # the key's QAP also holds the rows snarkjs adds for the public wires (one term each); at
            # least the unsplit partition's count (+ the empty class), at most half of the terms
            assert g["terms"] == 258327 + case.b.n_public + 1 and g["rows_grouped"]
            assert g["row_classes"] >= 6132 + 1 and 52188 <= g["terms_rep"] <= g["terms"] // 2
            assert g["wire_list"] > 0 and g["wires_over_cap"] == 0
        assert _check(key, res, case.abc[0]) == (0, 0, False)       # its own witness follows
        assert _check(key, res, case.abc[0], grouped=False) == (0, 0, False)
        other = key.upload(case.wts[1])
        miss, dirty, plain = _check(key, other, case.abc[1])
        if part != "learned":
            assert (miss, dirty, plain) == (0, 0, False)             # nothing to miss
        assert key.prove_resident(res, case.rs[0]) == case.proofs[0]


def test_misses_and_overflows(sgd, monkeypatch):
    """The learned partition under witnesses that miss a little and a lot, and a random pairing of the
    wires, which nearly every constraint misses: the list overflows and the plain ABC runs."""
    from zkfl import native
    _env(monkeypatch, {})
    with native.Context(0) as ctx:
        key = native.ProvingKey(ctx, sgd.zk)
        res = [key.upload(w) for w in sgd.wts]
        key.learn_groups(res[0])
        assert key.groups()["rows_grouped"]
        cap, miss_cap = max(64, sgd.dom // 8), max(64, sgd.dom // 64)
        few = _check(key, res[1], sgd.abc[1])
        many = _check(key, res[2], sgd.abc[2])
        print("client 2 (misses, dirty, plain)", few, "rotated rows", many, "capacities", cap, miss_cap)
        # counted here from the constraints: the wires that miss the partition learned from client 1
        # and the constraints they sit in (the key's split by query leaves these wires as they are)
        rep = _learned(sgd.w[0])

        def count(w):
            missing = {i for i in range(sgd.n) if w[i] != w[rep[i]]}
            return len(missing), sum(1 for A, B, _ in sgd.b.cons if missing & (A.keys() | B.keys()))

        assert count(sgd.w[1]) == (3, 14) and few == (3, 14, False)            # the issue's count
        # the rotation misses on more wires than the slot lists: the plain flag rises from the count
        # alone, no list is walked, nothing is marked
        assert count(sgd.w[2])[0] == 1455 > miss_cap and many == (1455, 0, True)
        # many dirty constraints under the capacities: client 1's witness with 150 non-representative
        # wires moved off their groups' values (a, b, c do not need a satisfying witness)
        from zkfl import zkey
        w = list(sgd.w[0])
        moved = [i for i in range(sgd.n) if rep[i] != i][::20][:150]
        assert len(moved) == 150
        for i in moved:
            w[i] = (w[i] + 1) % R
        n_miss, n_dirty = count(w)
        assert n_miss == 150 and 150 < n_dirty <= cap
        busy = _check(key, key.upload(zkey.wtns_bytes(w)), _abc_bytes(sgd.b, w, sgd.dom))
        print("150 wires moved: counted", (n_miss, n_dirty), "got", busy)
        assert not busy[2] and 150 <= busy[0] <= miss_cap and n_dirty <= busy[1] <= cap
        assert _check(key, res[0], sgd.abc[0]) == (0, 0, False)      # clean again after dirty runs
        # random pairs of wires
        rng = random.Random(5)
        order = list(range(1, sgd.n))
        rng.shuffle(order)
        rep = list(range(sgd.n))
        for x, y in zip(order[0::2], order[1::2]):
            rep[max(x, y)] = min(x, y)
        key.set_groups(rep)
        g = key.groups()
        miss, dirty, plain = _check(key, res[0], sgd.abc[0])
        print("random pairing:", g["non_rep"], "non-representative wires, misses", miss, "dirty", dirty, "plain", plain,
              "rows_grouped", g["rows_grouped"])
        assert g["rows_grouped"] and plain and miss > cap
        assert key.prove_resident(res[1], sgd.rs[1]) == sgd.proofs[1]


def test_a_and_b_rows_of_one_constraint_dirty(sgd, monkeypatch):
    """x * x constraints carry the same wire in their A and their B row: pairing such a wire with
    another of a different value dirties both rows of one constraint, and only those constraints."""
    from zkfl import native
    _env(monkeypatch, {})
    w = sgd.w[0]
    squares = [next(iter(A)) for A, B, _ in sgd.b.cons if A == B and len(A) == 1 and next(iter(A)) > 0]
    # the learned partition (which follows) with a squared wire y that was alone in its group
    # moved behind an earlier representative x of another value
    rep = _learned(w)
    heads = {r for i, r in enumerate(rep) if r != i}
    y = [i for i in squares if rep[i] == i and i not in heads][-1]
    touched = sum(1 for A, B, _ in sgd.b.cons if y in A or y in B)
    with native.Context(0) as ctx:
        key = native.ProvingKey(ctx, sgd.zk)
        res = key.upload(sgd.wts[0])
        key.set_groups(rep)
        n0 = key.groups()["non_rep"]
        for x in range(y - 1, max(0, y - 60), -1):   # a partner the key's split by query keeps
            if rep[x] != x or w[x] == w[y]:
                continue
            rep[y] = x
            key.set_groups(rep)
            if key.groups()["non_rep"] == n0 + 1:
                break
            rep[y] = y
        g = key.groups()
        assert g["non_rep"] == n0 + 1 and g["rows_grouped"]
        miss, dirty, plain = _check(key, res, sgd.abc[0])
        print("wire", y, "paired with", rep[y], ": misses", miss, "dirty", dirty, "constraints with the wire", touched)
        assert (miss, dirty, plain) == (1, touched, False)


def _learned(w):
    first, rep = {}, []
    for i, v in enumerate(w):
        rep.append(first.setdefault(v, i) if v >= 1 << 128 else i)
    return rep


def test_only_miss_in_the_last_constraint(sgd, monkeypatch):
    """A witness whose only miss sits in the last constraint: the last entry of the domain's real
    rows is recomputed and nothing else.  The witness need not satisfy the circuit for a, b, c."""
    from zkfl import native, zkey
    _env(monkeypatch, {})
    last = len(sgd.b.cons) - 1
    A, B, _ = sgd.b.cons[last]
    wires = sorted((set(A) | set(B)) - {0})
    assert wires
    w = sgd.w[0]
    # the learned partition, with a wire of the last constraint that was alone in its group moved
    # behind an earlier representative of another value: the one wire that misses
    rep = _learned(w)
    heads = {r for i, r in enumerate(rep) if r != i}
    x = [i for i in wires if rep[i] == i and i not in heads][-1]
    others = [j for j, (a, b, _) in enumerate(sgd.b.cons) if x in a or x in b]
    assert others[-1] == last
    with native.Context(0) as ctx:
        key = native.ProvingKey(ctx, sgd.zk)
        res = key.upload(sgd.wts[0])
        key.set_groups(rep)
        n0 = key.groups()["non_rep"]
        for twin in range(x - 1, max(0, x - 60), -1):   # a partner the key's split by query keeps
            if rep[twin] != twin or w[twin] == w[x]:
                continue
            rep[x] = twin
            key.set_groups(rep)
            if key.groups()["non_rep"] == n0 + 1:
                break
            rep[x] = x
        g = key.groups()
        assert g["non_rep"] == n0 + 1 and g["rows_grouped"]
        miss, dirty, plain = _check(key, res, sgd.abc[0])
        print("last constraint", last, "wire", x, "behind", rep[x], "sits in constraints", others, "misses", miss,
              "dirty", dirty)
        assert (miss, dirty, plain) == (1, len(others), False)


def test_wire_over_the_cap_runs_the_plain_form(sgd, monkeypatch):
    """A non-representative wire in more constraints than the cap carries no list; when it misses the
    proof runs the plain ABC, when it follows nothing is dirty."""
    from zkfl import native, zkey
    fan = [0] * sgd.n
    for A, B, _ in sgd.b.cons:
        for i in set(A) | set(B):
            fan[i] += 1
    h = max(range(1, sgd.n), key=lambda i: fan[i])
    assert 100 < fan[h] <= 256
    _env(monkeypatch, {"ZKFL_GROUP_ROWS_CAP": "100"})
    w = sgd.w[0]
    with native.Context(0) as ctx:
        key = native.ProvingKey(ctx, sgd.zk)
        res = key.upload(sgd.wts[0])
        rep = _learned(w)
        assert rep[h] == h
        key.set_groups(rep)
        over0 = key.groups()["wires_over_cap"]       # learned twins of such wires are over this cap too,
        assert _check(key, res, sgd.abc[0]) == (0, 0, False)   # and follow: nothing is raised
        g0 = None
        for twin in range(h - 1, max(0, h - 60), -1):   # a partner the key's split by query keeps
            if rep[twin] != twin or w[twin] == w[h]:
                continue
            rep[h] = twin
            key.set_groups(rep)
            g0 = key.groups()
            if g0["wires_over_cap"] == over0 + 1:
                break
            rep[h] = h
        assert g0 and g0["wires_over_cap"] == over0 + 1 and g0["rows_grouped"]
        miss, dirty, plain = _check(key, res, sgd.abc[0])
        print("wire", h, "in", fan[h], "constraints, paired with", rep[h], ": misses", miss, "dirty", dirty)
        assert miss == 1 and plain
        assert key.prove_resident(res, sgd.rs[0]) == sgd.proofs[0]
        # the same wire following its partner: nothing dirty, the grouped form runs
        w2 = list(w)
        w2[h] = w2[rep[h]]
        follow = key.upload(zkey.wtns_bytes(w2))
        assert _check(key, follow, _abc_bytes(sgd.b, w2, sgd.dom)) == (0, 0, False)


def test_group_rows_off_keeps_the_plain_abc(sgd, monkeypatch):
    from zkfl import native
    _env(monkeypatch, {"ZKFL_GROUP_ROWS": "0"})
    with native.Context(0) as ctx:
        key = native.ProvingKey(ctx, sgd.zk)
        res = [key.upload(w) for w in sgd.wts[:2]]
        key.learn_groups(res[0])
        g = key.groups()
        assert g["grouped"] and not g["rows_grouped"] and g["row_classes"] == 0
        for i in (0, 1):
            miss, dirty, plain = _check(key, res[i], sgd.abc[i])
            assert (dirty, plain) == (0, False)
            assert key.prove_resident(res[i], sgd.rs[i]) == sgd.proofs[i]


def test_batch_of_twelve_resets_between_proofs(sgd, monkeypatch):
    """12 proofs on a 2-slot key, the clean and the client-2 witness alternating (each slot's graph is
    captured on its second proof and replayed after), then the same in pairs so that each slot
    itself alternates; then batches of two whose last proof alternates, read back through the key's
    report: a dirty proof must leave nothing behind for the clean one after it."""
    from zkfl import native
    _env(monkeypatch, {"ZKFL_SMALL_LOGN": "0"})
    with native.Context(0) as ctx:
        key = native.ProvingKey(ctx, sgd.zk)
        key.set_slots(2)
        res = [key.upload(w) for w in sgd.wts[:2]]
        key.learn_groups(res[0])
        assert key.groups()["rows_grouped"]
        for which in ([0, 1] * 6, [0, 1, 1, 0] * 3):
            got = key.prove_batch([res[i] for i in which], b"".join(sgd.rs[i] for i in which))
            assert got == [sgd.proofs[i] for i in which]
        dirty = []
        for t in range(6):
            which = [0, 1] if t % 2 == 0 else [1, 0]
            got = key.prove_batch([res[i] for i in which], b"".join(sgd.rs[i] for i in which))
            assert got == [sgd.proofs[i] for i in which]
            g = key.groups()
            assert not g["last_plain"]
            dirty.append(g["last_dirty"])                # of slot 1's proof, the last one waited for
        print("dirty counts of slot 1's proofs:", dirty)
        assert dirty[1::2] == [0, 0, 0] and all(d > 0 for d in dirty[0::2]) and len(set(dirty[0::2])) == 1
        assert _check(key, res[0], sgd.abc[0]) == (0, 0, False)


@pytest.mark.parametrize("small_logn", [None, "0"], ids=["front", "chain"])
def test_one_proof_alone_and_small_key_schedules(sgd, monkeypatch, small_logn):
    """One proof alone after set_groups (the latency schedule) and a batch over the learned
    partition, clean and with misses: as a small key (the default: the front schedule, which keeps
    the plain ABC and builds no row classes) and as a large one (the chain, grouped ABC)."""
    from zkfl import native
    _env(monkeypatch, {}, small_logn=small_logn)
    with native.Context(0) as ctx:
        key = native.ProvingKey(ctx, sgd.zk)
        res = [key.upload(w) for w in sgd.wts[:2]]
        key.set_groups(_learned(sgd.w[0]))
        g = key.groups()
        assert g["grouped"] and g["rows_grouped"] == (small_logn == "0")
        assert g["row_classes"] == (0 if small_logn is None else g["row_classes"]) and (small_logn is None or g["row_classes"])
        assert key.prove_resident(res[1], sgd.rs[1]) == sgd.proofs[1]
        assert key.groups()["last_dirty"] == (14 if small_logn == "0" else 0)
        assert key.prove_resident(res[0], sgd.rs[0]) == sgd.proofs[0]
        assert key.groups()["last_dirty"] == 0
        key.set_slots(2)
        which = [0, 1, 1, 0, 0, 1]
        got = key.prove_batch([res[i] for i in which], b"".join(sgd.rs[i] for i in which))
        assert got == [sgd.proofs[i] for i in which]
