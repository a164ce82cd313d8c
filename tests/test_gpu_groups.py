"""Grouped form of the witness queries: one MSM base per group of wires that carry equal values
(csrc/groups.h) -- MI355X (-m gpu).

For ANY partition of the wires, sum_i w_i P_i = sum_g w_rep(g) S_g + sum_{i non-rep} (w_i - w_rep(i)) P_i,
so a partition can only change how fast a proof is computed.  The bar everywhere is byte equality:
with the same key's proofs after the partition is dropped, and with the C oracle
(oracle/c/groth16_ref.c), for fixed (r, s).

Circuits: poseidon_hash2 (the smallest) and sgd_verified(8, 4, 3, 1000); 14-bit windows (small
keys' default) and one case at 16 bits.  The options are read when a context is created and the
window width when a key loads, so every setting opens a context of its own.

The learned partition (client 1 of sgd_verified(8, 4, 3)) measured on the CPU oracle: 4,122
non-representative wires in 1,702 groups; clients 2 and 3 miss on 3 and 4 of them.  Reversing the
sample rows of client 1's input does NOT break the pattern (3 misses): i -> 7 - i maps the tree onto
itself, so samples still share their nodes pairwise.  Rotating the rows by one does (1,455 misses),
so the many-misses case is the rotation; the reversal is kept as a case that still follows.
"""
import random

import pytest

pytestmark = pytest.mark.gpu

KNOBS = ("ZKFL_GRAPH", "ZKFL_STAGGER", "ZKFL_LOWLAT", "ZKFL_FAST_WSUM", "ZKFL_SMALL_LOGN", "ZKFL_AB_SHARED",
         "ZKFL_GROUPS", "ZKFL_GROUP_MIN_BATCH", "ZKFL_MSM_C")
TAU_SQ = 100000000


def _le(x):
    return int(x).to_bytes(32, "little")


def _env(monkeypatch, setting):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, value in setting.items():
        monkeypatch.setenv(name, value)


def _permuted(inp, perm):
    out = dict(inp)
    for k in ("features", "labels", "siblings", "pathIndices"):
        out[k] = [inp[k][p] for p in perm]
    return out


class Case:
    """A circuit, its key bytes, witnesses (values and .wtns bytes), one (r, s) per witness and the
    C oracle's proofs, computed once and left unchanged."""

    def __init__(self, ctx, b, inputs, seed):
        from oracle import bn254 as bn
        from oracle import cbaseline
        from oracle import witness as ow
        from zkfl import zkey
        self.b = b
        self.zk = zkey.groth16_setup(b, ctx, zkey.Toxic(tau=seed, alpha=seed + 1, beta=seed + 2, gamma=seed + 3,
                                                       delta=seed + 4))
        self.w = [ow.evaluate(b, i) for i in inputs]
        self.wts = [zkey.wtns_bytes(w) for w in self.w]
        pool = [_le(0x1234567) + _le(0x7654321), _le(bn.R - 1) + _le(bn.R - 2), _le(3) + _le(bn.R - 1)]
        self.rs = [pool[i % 3] for i in range(len(inputs))]
        self.proofs = [cbaseline.prove(self.zk, w, r) for w, r in zip(self.wts, self.rs)]
        self.n = len(self.w[0])


@pytest.fixture(scope="module")
def hash2(gpu_ctx):
    from oracle import bn254 as bn
    from zkfl import circuits
    ins = [{"left": 1, "right": 2}, {"left": bn.R - 1, "right": 5}, {"left": 0, "right": 0}]
    return Case(gpu_ctx, circuits.build("poseidon_hash2"), ins, 0x6A1)


@pytest.fixture(scope="module")
def sgd(gpu_ctx):
    """witnesses 0..2: clients 1..3; 3: client 1 with its sample rows reversed; 4: rotated by one;
    5: a client whose eight samples are one and the same row (every leaf and path equal: 7,336
    non-representative wires, of which clients 1 and 2 miss 4,683 and 4,671, CPU oracle)"""
    from zkfl import circuits, clients
    ins = [clients.Client(cid, 8, 4, 3, clients.JsLcg(12345)).training_input(8, 1000, TAU_SQ)[0] for cid in (1, 2, 3)]
    ins += [_permuted(ins[0], list(range(7, -1, -1))), _permuted(ins[0], [1, 2, 3, 4, 5, 6, 7, 0])]
    c = clients.Client(1, 8, 4, 3, clients.JsLcg(12345))
    c.features, c.labels = [c.features[0]] * 8, [c.labels[0]] * 8
    c.tree = clients.merkle_tree([clients.vector_hash(f + [l]) for f, l in zip(c.features, c.labels)], 3)
    c.root_D = c.tree.root
    ins.append(c.training_input(8, 1000, TAU_SQ)[0])
    return Case(gpu_ctx, circuits.build("sgd_verified", 8, 4, 3, 1000), ins, 0x6B2)


def _partition(name, case):
    n, w = case.n, case.w
    if name == "identity":
        return list(range(n))
    if name == "neighbours":
        return [i & ~1 for i in range(n)]
    if name == "random":          # groups of 1..9 wires drawn from all over the witness
        rng = random.Random(n)
        order = list(range(n))
        rng.shuffle(order)
        rep, k = [0] * n, 0
        while k < n:
            g = order[k:k + rng.randint(1, 9)]
            for i in g:
                rep[i] = min(g)
            k += len(g)
        return rep
    if name == "all":
        return [0] * n
    if name == "zeros":           # wires with value 0 in a witness behind a non-zero first wire, and the
        rep = list(range(n))      # other way round: u = 0 - w_rep wraps mod r, u = w_i - 0 is full width
        zeros = [i for i in range(1, n) if any(w[k][i] == 0 for k in range(3))]
        assert len(zeros) >= 2
        for i in zeros[:len(zeros) // 2]:
            rep[i] = 0            # wire 0 carries 1
        z = zeros[len(zeros) // 2]
        for i in range(z + 1, n):
            if rep[i] == i and i % 3 == 0:
                rep[i] = z
        return rep
    raise KeyError(name)


def _prove_three(key, case, which=(0, 1, 2)):
    res = [key.upload(case.wts[i]) for i in which]
    got = key.prove_batch(res, b"".join(case.rs[i] for i in which))
    for r in res:
        r.close()
    return got


def _check_partition(case, key, rep):
    want = [case.proofs[i] for i in (0, 1, 2)]
    key.set_groups(rep)
    g = key.groups()
    assert g["grouped"] and not g["learned"]
    # the key splits a group whose first wire lacks a base in a query where a member has one
    asked = sum(1 for i, r in enumerate(rep) if r != i)
    assert g["non_rep"] <= asked
    print("non-representative wires asked", asked, "kept", g["non_rep"])
    got = _prove_three(key, case)
    misses = key.groups()["last_miss"]
    single = key.prove(case.wts[0], case.rs[0])[0]          # a batch of one: the latency schedule
    key.set_groups(None)
    assert not key.groups()["grouped"]
    plain = _prove_three(key, case)
    assert got == plain, "the partition changed proof bytes"
    assert got == want and single == want[0], "proofs differ from the C oracle"
    return misses


CASES = [("hash2", "identity"), ("hash2", "neighbours"), ("hash2", "random"), ("hash2", "all"), ("hash2", "zeros"),
         ("sgd", "identity"), ("sgd", "neighbours"), ("sgd", "random"), ("sgd", "zeros")]


@pytest.mark.parametrize("circuit,part", CASES, ids=[f"{c}-{p}" for c, p in CASES])
def test_any_partition_gives_the_same_bytes(request, monkeypatch, circuit, part):
    from zkfl import native
    case = request.getfixturevalue(circuit)
    rep = _partition(part, case)
    _env(monkeypatch, {})
    with native.Context(0) as ctx:
        key = native.ProvingKey(ctx, case.zk)
        misses = _check_partition(case, key, rep)
        if part == "identity":
            assert misses == 0
        if part in ("neighbours", "random", "all"):
            assert misses > 0      # arbitrary pairings of a witness do not hold


def test_sixteen_bit_windows(sgd, monkeypatch):
    from zkfl import native
    _env(monkeypatch, {"ZKFL_MSM_C": "16"})
    with native.Context(0) as ctx:
        key = native.ProvingKey(ctx, sgd.zk)
        _check_partition(sgd, key, _partition("random", sgd))
        _check_partition(sgd, key, _partition("zeros", sgd))


def test_learned_partition(sgd, monkeypatch):
    """Learned from client 1: it follows with no miss, clients 2 and 3 and the reversed rows with a
    few, the rotated rows with many -- every proof the oracle's bytes."""
    from zkfl import native
    _env(monkeypatch, {})
    with native.Context(0) as ctx:
        key = native.ProvingKey(ctx, sgd.zk)
        res = [key.upload(w) for w in sgd.wts]
        key.learn_groups(res[0])
        g = key.groups()
        assert g["grouped"] and g["learned"] and g["non_rep"] > 0 and 0 < g["groups"] <= g["non_rep"]
        for q in ("A", "B1", "B2", "CH"):
            assert g["bases_rep"][q] < g["bases"][q]
        assert g["bases"]["B1"] == g["bases"]["B2"] and g["bases_rep"]["B1"] == g["bases_rep"]["B2"]
        # what the host model of tests/test_groups_cpu.py says of the same witness
        first, model = {}, 0
        for i, v in enumerate(sgd.w[0]):
            model += first.setdefault(v, i) != i if v >= 1 << 128 else 0
        assert model // 2 < g["non_rep"] <= model     # twins have equal roles: the split by query costs little
        misses = []
        for i in range(5):
            assert key.prove_resident(res[i], sgd.rs[i]) == sgd.proofs[i], f"witness {i}"
            misses.append(key.groups()["last_miss"])
        print("non-representative wires", g["non_rep"], "misses", misses)
        assert misses[0] == 0
        assert 0 < misses[1] < g["non_rep"] // 20 and 0 < misses[2] < g["non_rep"] // 20
        assert misses[3] < g["non_rep"] // 20           # the reversal maps the tree onto itself
        assert 4 * misses[4] > g["non_rep"]             # the rotation does not
        # the same five as one batch on two slots: launch by launch, then graph replay
        key.set_slots(2)
        assert key.prove_batch(res, b"".join(sgd.rs)) == sgd.proofs
        assert key.groups()["builds"] == 1


SETTINGS = [{"ZKFL_SMALL_LOGN": "0"}, {"ZKFL_SMALL_LOGN": "0", "ZKFL_GRAPH": "0"}, {"ZKFL_LOWLAT": "0"},
            {"ZKFL_SMALL_LOGN": "0", "ZKFL_STAGGER": "0"}]


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: ",".join(f"{k}={v}" for k, v in s.items()))
def test_other_schedules_run_the_grouped_form(sgd, monkeypatch, setting):
    """The large-key chain (staggered and not, replayed and launch by launch) and a batch of one on
    the one-stream schedule, over the learned partition and over one that mostly misses."""
    from zkfl import native
    _env(monkeypatch, setting)
    with native.Context(0) as ctx:
        key = native.ProvingKey(ctx, sgd.zk)
        key.set_slots(2)
        res = [key.upload(w) for w in sgd.wts]
        for rep in (None, _partition("random", sgd)):
            if rep is None:
                key.learn_groups(res[0])
            else:
                key.set_groups(rep)
            assert key.groups()["grouped"]
            assert key.prove_batch(res + res, b"".join(sgd.rs) * 2) == sgd.proofs * 2
            assert key.prove_resident(res[1], sgd.rs[1]) == sgd.proofs[1]


def test_batch_of_nine_learns_and_replays(sgd, monkeypatch):
    """The default threshold: a batch of 9 on 2 slots learns from its first witness before
    anything is enqueued, then runs the front schedule, graph replay from each slot's second
    proof; smaller batches before it do not learn."""
    from zkfl import native
    _env(monkeypatch, {})
    with native.Context(0) as ctx:
        key = native.ProvingKey(ctx, sgd.zk)
        key.set_slots(2)
        assert _prove_three(key, sgd) == sgd.proofs[:3]
        assert key.prove(sgd.wts[1], sgd.rs[1])[0] == sgd.proofs[1]
        assert not key.groups()["grouped"] and key.groups()["builds"] == 0
        which = [0, 1, 2, 3, 4, 0, 1, 0, 0]
        res = [key.upload(sgd.wts[i]) for i in which]
        got = key.prove_batch(res, b"".join(sgd.rs[i] for i in which))
        assert got == [sgd.proofs[i] for i in which]
        g = key.groups()
        assert g["grouped"] and g["learned"] and g["builds"] == 1 and g["non_rep"] > 0 and g["build_ms"] > 0
        assert g["last_miss"] == 0                       # both slots' last proofs are client 1's
        # the key keeps its partition: another batch does not learn again
        assert key.prove_batch(res, b"".join(sgd.rs[i] for i in which)) == got
        assert key.groups()["builds"] == 1


def test_relearns_when_most_wires_miss(sgd, monkeypatch):
    """A learned partition that misses on more than half of its wires in the key's last proof is
    learned again at the start of the next batch call, once."""
    from zkfl import native
    _env(monkeypatch, {"ZKFL_GROUP_MIN_BATCH": "2"})
    with native.Context(0) as ctx:
        key = native.ProvingKey(ctx, sgd.zk)
        res = [key.upload(w) for w in sgd.wts]
        # learned from the witness of eight equal rows: far more groups than the workload has
        assert key.prove_batch([res[5], res[5]], sgd.rs[5] * 2) == [sgd.proofs[5]] * 2
        g0 = key.groups()
        assert g0["learned"] and g0["builds"] == 1 and g0["last_miss"] == 0
        # real clients miss on most of them; the call that sees it first does not learn (nothing had
        # missed when it started)
        assert key.prove_batch([res[0], res[1]], sgd.rs[0] + sgd.rs[1]) == sgd.proofs[:2]
        g1 = key.groups()
        print("equal-rows partition:", g0["non_rep"], "wires; client 2 misses", g1["last_miss"])
        assert g1["builds"] == 1 and 2 * g1["last_miss"] > g1["non_rep"]
        # the next one does, from its first witness (client 1), and only once
        assert key.prove_batch([res[0], res[1], res[2]], b"".join(sgd.rs[:3])) == sgd.proofs[:3]
        g2 = key.groups()
        assert g2["builds"] == 2 and g2["non_rep"] < g0["non_rep"] and g2["last_miss"] < g2["non_rep"] // 20
        # a single proof never learns, whatever missed before it
        key.set_groups(None)
        assert key.prove_resident(res[0], sgd.rs[0]) == sgd.proofs[0]
        assert not key.groups()["grouped"]


def test_groups_off_never_groups(sgd, monkeypatch):
    from zkfl import native
    _env(monkeypatch, {"ZKFL_GROUPS": "0"})
    with native.Context(0) as ctx:
        key = native.ProvingKey(ctx, sgd.zk)
        key.set_slots(2)
        which = [0, 1, 2, 3, 4, 0, 1, 2, 0]
        res = [key.upload(sgd.wts[i]) for i in which]
        assert key.prove_batch(res, b"".join(sgd.rs[i] for i in which)) == [sgd.proofs[i] for i in which]
        g = key.groups()
        assert not g["grouped"] and g["builds"] == 0
        with pytest.raises(native.ZkflError) as e:
            key.set_groups(list(range(sgd.n)))
        assert e.value.code == -1
        with pytest.raises(native.ZkflError):
            key.learn_groups(res[0])
        key.set_groups(None)


def test_argument_errors(hash2, monkeypatch):
    from zkfl import native
    _env(monkeypatch, {})
    n = hash2.n
    with native.Context(0) as ctx:
        key = native.ProvingKey(ctx, hash2.zk)
        bad = [list(range(n)) for _ in range(3)]
        bad[0][3] = 5                       # rep[i] > i
        bad[1][4], bad[1][6] = 2, 4         # rep[rep[6]] = 2 != rep[6]
        bad[2] = bad[2][:-1]                # wrong length
        for rep in bad + [list(range(n)) + [0]]:
            with pytest.raises(native.ZkflError) as e:
                key.set_groups(rep)
            assert e.value.code == -1
        assert not key.groups()["grouped"]
        shard = native.ProvingKey(ctx, hash2.zk, shard=0, n_shards=2)
        with pytest.raises(native.ZkflError) as e:
            shard.set_groups(list(range(n)))
        assert e.value.code == -1
        assert key.prove(hash2.wts[0], hash2.rs[0])[0] == hash2.proofs[0]
