"""The A query in D form: A = B1 + sum w_i (A_i - B1_i) -- MI355X (-m gpu).

A wire whose A and B columns of the QAP are equal (x * x = y, x used nowhere else) has the same G1
point in the A and the B1 section of the key, and both MSMs multiply it by the same scalar.  The
loader compares the two sections byte for byte and, where that leaves fewer bases, loads
D_i = A_i - B1_i in A's place (csrc/key_load.hip, csrc/host_parse.cc ab_partition); a proof then adds
B1's result to D's (csrc/assemble.hip k_fold_a).  Nothing about results may change.

The systems are hand-built (zkfl.r1cs.Builder, domain 16) so that every wire kind is there:
  main        t in B only | x[5] squares: equal columns, dropped | u with B = -A (P - Q a doubling) |
              v in A only | s in both, different | p public | the products and `out` in A only
  b_heavy     one square against two B-only wires: the A form is kept
  all_shared  every wire with a B1 base is a square: D holds A-only wires and the augmentation
and the bar is byte equality with the C oracle (oracle/c/groth16_ref.c).  The options are read when
a context is created, so every setting opens a context of its own.
"""
import pytest

pytestmark = pytest.mark.gpu

KNOBS = ("ZKFL_GRAPH", "ZKFL_STAGGER", "ZKFL_LOWLAT", "ZKFL_FAST_WSUM", "ZKFL_SMALL_LOGN", "ZKFL_AB_SHARED")
TOXIC = dict(tau=0x5C4ED, alpha=0xA1, beta=0xB2, gamma=0xC3, delta=0xD4)
MAIN_SHARED = 5


def _le(x):
    return int(x).to_bytes(32, "little")


def _main():
    from zkfl import r1cs
    b = r1cs.Builder("ab_main")
    out = b.output("out")
    p = b.input("p", public=True)
    t = b.input("t")
    x = b.input("x", (MAIN_SHARED,))
    u, v, s = b.input("u"), b.input("v"), b.input("s")
    prods = [b.mul(xi, xi) for xi in x]
    prods.append(b.mul(u, r1cs.scale(u, r1cs.R - 1)))
    prods.append(b.mul(v, t))
    prods.append(b.mul(r1cs.add(s, p), r1cs.scale(s, 3)))
    b.bind_output(out, r1cs.lc_sum(prods))
    ins = [dict(p=7, t=11, x=[3, 5, r1cs.R - 2, 1 << 200, 12345], u=13, v=17, s=19),
           dict(p=r1cs.R - 1, t=2, x=[9, 8, 7, 6, 5], u=1 << 250, v=4, s=r1cs.R - 3)]
    return b, ins


def _b_heavy():
    from zkfl import r1cs
    b = r1cs.Builder("ab_b_heavy")
    out = b.output("out")
    p = b.input("p", public=True)
    x, v, t = b.input("x"), b.input("v", (2,)), b.input("t", (2,))
    prods = [b.mul(r1cs.add(x, p), x), b.mul(v[0], t[0]), b.mul(v[1], t[1])]
    b.bind_output(out, r1cs.lc_sum(prods))
    return b, [dict(p=3, x=5, v=[7, 9], t=[11, 13])]


def _all_shared():
    from zkfl import r1cs
    b = r1cs.Builder("ab_all_shared")
    p = b.input("p", public=True)
    x = b.input("x", (3,))
    b.mul(r1cs.add(x[0], p), x[0])
    b.mul(x[1], x[1])
    b.mul(x[2], x[2])
    return b, [dict(p=21, x=[2, r1cs.R - 5, 1 << 100])]


def _columns(b):
    """-> (A, B): per wire {row: coef} as the key's sections 5 and 6 see them (snarkjs adds the
    rows n_cons + k: wire k, to A for the public wires)."""
    A = [dict() for _ in range(b.n_wires)]
    B = [dict() for _ in range(b.n_wires)]
    for j, (a, bb, _c) in enumerate(b.cons):
        for w, c in a.items():
            A[w][j] = c
        for w, c in bb.items():
            B[w][j] = c
    for k in range(b.n_public + 1):
        A[k][len(b.cons) + k] = 1
    return A, B


def _counts(b, shard=0, n_shards=1):
    """-> (shared wires, form) of a shard by the loader's rule: D when its image (wires whose
    columns differ, + 3 augmentation pairs on shard 0) has fewer bases than A's (+ 2)."""
    A, B = _columns(b)
    mine = range(shard, b.n_wires, n_shards)
    shared = sum(1 for i in mine if A[i] and A[i] == B[i])
    n_a = sum(1 for i in mine if A[i]) + (2 if shard == 0 else 0)
    n_d = sum(1 for i in mine if A[i] != B[i]) + (3 if shard == 0 else 0)
    return shared, "D" if n_d < n_a else "A"


class Case:
    def __init__(self, ctx, build, toxic=TOXIC):
        from oracle import bn254 as bn
        from oracle import cbaseline
        from oracle import witness as ow
        from zkfl import zkey
        self.b, ins = build()
        self.zk = zkey.groth16_setup(self.b, ctx, zkey.Toxic(**toxic))
        self.wts = [zkey.wtns_bytes(ow.evaluate(self.b, i)) for i in ins]
        # r, s from {small, r - 1, r - 2}
        self.rs = [_le(0x1234567) + _le(0x7654321), _le(bn.R - 1) + _le(bn.R - 2), _le(bn.R - 2) + _le(5),
                   _le(3) + _le(bn.R - 1)]
        self.which = [i % len(self.wts) for i in range(len(self.rs))]
        self.proofs = [cbaseline.prove(self.zk, self.wts[w], r) for w, r in zip(self.which, self.rs)]
        self.domain = zkey.domain_size_for(self.b)
        _, self.h, self.parts = cbaseline.prove_parts(self.zk, self.wts[0], self.rs[0], self.domain)


@pytest.fixture(scope="module")
def main_case(gpu_ctx):
    return Case(gpu_ctx, _main)


def _env(monkeypatch, setting):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, value in setting.items():
        monkeypatch.setenv(name, value)


def _check_key(case, key, parts=True):
    """Every proof of the case alone (a batch of one), the four as one batch on two slots (each
    slot proves launch by launch, then replays its graph), and the parity hook's five MSMs."""
    for w, r, want in zip(case.which, case.rs, case.proofs):
        assert key.prove(case.wts[w], r)[0] == want, "a batch of one differs from the oracle"
    key.set_slots(2)
    res = [key.upload(w) for w in case.wts]
    got = key.prove_batch([res[w] for w in case.which], b"".join(case.rs))
    for w in res:
        w.close()
    assert got == case.proofs, "the batch of four on two slots differs from the oracle"
    if parts:
        hs, got_parts = key.debug_parts(case.wts[0])
        assert hs == case.h
        for name in ("A", "B1", "B2", "C", "H"):
            assert got_parts[name] == case.parts[name], f"MSM {name} differs"


SETTINGS = [{}, {"ZKFL_SMALL_LOGN": "0"}, {"ZKFL_SMALL_LOGN": "0", "ZKFL_GRAPH": "0"}, {"ZKFL_LOWLAT": "0"}]


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: ",".join(f"{k}={v}" for k, v in s.items()) or "default")
def test_d_form_proves_the_oracle_bytes(main_case, monkeypatch, setting):
    """1 and 3: the main system loads in D form with the shared wires it was built with, and the
    latency, front and chain schedules prove the oracle's bytes and parts."""
    from zkfl import native
    assert _counts(main_case.b) == (MAIN_SHARED, "D")
    _env(monkeypatch, setting)
    with native.Context(0) as ctx:
        key = native.ProvingKey(ctx, main_case.zk)
        info = key.ab_shared()
        assert info["form"] == "D" and info["shared_wires"] == MAIN_SHARED
        A, B = _columns(main_case.b)
        assert info["a_bases"] == sum(1 for a, b in zip(A, B) if a != b) + 3
        _check_key(main_case, key)


@pytest.mark.parametrize("small_logn", ["16", "0"])
def test_option_off_proves_the_same_bytes(main_case, monkeypatch, small_logn):
    """2: ZKFL_AB_SHARED=0 keeps the A form; the same (witness, r, s) give the same bytes."""
    from zkfl import native
    got = {}
    for on in ("1", "0"):
        _env(monkeypatch, {"ZKFL_AB_SHARED": on, "ZKFL_SMALL_LOGN": small_logn})
        with native.Context(0) as ctx:
            key = native.ProvingKey(ctx, main_case.zk)
            assert key.ab_shared()["form"] == ("D" if on == "1" else "A")
            res = [key.upload(w) for w in main_case.wts]
            got[on] = [key.prove(main_case.wts[w], r)[0] for w, r in zip(main_case.which, main_case.rs)]
            got[on] += key.prove_batch([res[w] for w in main_case.which], b"".join(main_case.rs))
    assert got["1"] == got["0"] == main_case.proofs * 2


def test_b_heavy_key_keeps_the_a_form(gpu_ctx, monkeypatch):
    """3: one shared wire against two B-only wires: D would have more bases, so A stays."""
    from zkfl import native
    case = Case(gpu_ctx, _b_heavy)
    assert _counts(case.b) == (1, "A")
    _env(monkeypatch, {})
    with native.Context(0) as ctx:
        key = native.ProvingKey(ctx, case.zk)
        info = key.ab_shared()
        assert info["form"] == "A" and info["shared_wires"] == 1
        _check_key(case, key)


def test_alpha_equals_beta(gpu_ctx, monkeypatch):
    """4: alpha == beta makes the augmentation base alpha1 - beta1 the point at infinity."""
    from zkfl import native
    case = Case(gpu_ctx, _main, dict(TOXIC, beta=TOXIC["alpha"]))
    _env(monkeypatch, {})
    with native.Context(0) as ctx:
        key = native.ProvingKey(ctx, case.zk)
        assert key.ab_shared()["form"] == "D"
        _check_key(case, key)


def test_every_b_wire_shared(gpu_ctx, monkeypatch):
    """5: D is the A-only wires and the augmentation."""
    from zkfl import native
    case = Case(gpu_ctx, _all_shared)
    A, B = _columns(case.b)
    assert all(A[i] == B[i] for i in range(case.b.n_wires) if B[i]) and _counts(case.b) == (3, "D")
    _env(monkeypatch, {})
    with native.Context(0) as ctx:
        key = native.ProvingKey(ctx, case.zk)
        info = key.ab_shared()
        assert info == {"form": "D", "shared_wires": 3, "a_bases": sum(1 for a, b in zip(A, B) if a and not b) + 3}
        _check_key(case, key)


@pytest.mark.parametrize("world", [2, 3])
def test_shards_sum_to_the_unsplit_proof(gpu_ctx, main_case, monkeypatch, world):
    """6: each shard decides for itself (shard 0 alone carries the augmentation); the parts, summed
    and assembled as tests/test_gpu_split.py does, are the unsplit proof and the oracle's."""
    from zkfl import native
    _env(monkeypatch, {})
    want = [_counts(main_case.b, k, world) for k in range(world)]
    assert sum(c for c, _ in want) == MAIN_SHARED and "D" in [f for _, f in want]
    rs = b"".join(main_case.rs)
    with native.Context(0) as ctx:
        keys = [native.ProvingKey(ctx, main_case.zk, shard=k, n_shards=world) for k in range(world)]
        parts = []
        for k, key in enumerate(keys):
            info = key.ab_shared()
            assert (info["shared_wires"], info["form"]) == want[k], f"shard {k}"
            ws = [key.upload(main_case.wts[w]) for w in main_case.which]
            parts.append(key.prove_part_batch(ws, rs))
        blob = b"".join(parts[k][i] for i in range(len(main_case.rs)) for k in range(world))
        proofs = ctx.assemble(blob, world, rs)
        full = native.ProvingKey(ctx, main_case.zk)
        ws = [full.upload(main_case.wts[w]) for w in main_case.which]
        assert proofs == full.prove_batch(ws, rs) == main_case.proofs


def test_c2_loads_in_d_form(gpu_ctx, monkeypatch):
    """config 5's training circuit sgd_verified(8, 4, 3, 1000): 3,134 of its 6,712 B1 wires are
    S-box squares."""
    from zkfl import circuits, native, zkey
    b = circuits.build("sgd_verified", 8, 4, 3, 1000)
    assert _counts(b) == (3134, "D")
    zk = zkey.groth16_setup(b, gpu_ctx, zkey.Toxic(**TOXIC))
    _env(monkeypatch, {})
    with native.Context(0) as ctx:
        key = native.ProvingKey(ctx, zk)
        info = key.ab_shared()
        assert info["form"] == "D" and info["shared_wires"] == 3134
