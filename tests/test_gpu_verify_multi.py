"""Multi-key verification (zkfl_vkey_*, zkfl_groth16_verify_multi) and the wave verifier
(one proof per wavefront, csrc/verify_wave.hip) — MI355X.

Bar: the wave path's Miller values and GT elements are the lane path's byte for byte, and
oracle/pairing_tower.py's on the items the slow Python tower is asked about; verdicts under
"waves", "lanes" and "auto" are equal to each other, to the expected list per tamper kind, and to
oracle/groth16.py::verify on one valid and one invalid job per key.
"""
import json
import os
import random
import subprocess
import sys

import pytest

from oracle import bn254 as bn
from oracle import groth16 as og
from oracle import pairing_tower as T
from oracle import witness as ow

pytestmark = pytest.mark.gpu

R, Q = bn.R, bn.Q
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _le(x):
    return int(x).to_bytes(32, "little")


def _g1b(P):
    return bn.g1_to_bytes_std(P)


def _g2b(Qg):
    return bn.g2_to_bytes_std(Qg)


def _fq2_sqrt(a):
    """sqrt in Fq2 (q = 3 mod 4) or None."""
    a0, a1 = a.c0, a.c1
    n = (a0 * a0 + a1 * a1) % Q
    s = pow(n, (Q + 1) // 4, Q)
    if s * s % Q != n:
        return None
    for t in (s, -s % Q):
        x0sq = (a0 + t) * pow(2, -1, Q) % Q
        x0 = pow(x0sq, (Q + 1) // 4, Q)
        if x0 * x0 % Q == x0sq and x0:
            x1 = a1 * pow(2 * x0, -1, Q) % Q
            r = bn.Fq2(x0, x1)
            if r * r == a:
                return r
    return None


def _twist_point_outside_g2(seed=5):
    """A point on y^2 = x^3 + b' over Fq2 that is not in the order-r subgroup ([r]P != O)."""
    x = seed
    while True:
        X = bn.Fq2(x, 1)
        Y = _fq2_sqrt(X * X * X + bn.B2)
        if Y is not None:
            P = (X, Y)
            assert bn.on_curve(P)
            acc, base, k = None, bn.to_jac(P), R
            while k:
                if k & 1:
                    acc = bn.jadd(acc, base)
                base = bn.jdouble(base)
                k >>= 1
            if bn.from_jac(acc) is not None:
                return P
        x += 1


@pytest.fixture(scope="module")
def outside_g2():
    return _g2b(_twist_point_outside_g2())


# ---------------------------------------------------------------------------
# 1. wave pairing parity
# ---------------------------------------------------------------------------
def test_wave_pairing_bit_exact_vs_lanes_and_tower(gpu_ctx):
    rng = random.Random(11)
    Ps = [bn.G1_GEN] + [bn.mul(bn.G1_GEN, rng.randrange(1, R)) for _ in range(4)]
    Qs = [bn.G2_GEN] + [bn.mul(bn.G2_GEN, rng.randrange(1, R)) for _ in range(4)]
    g1 = b"".join(_g1b(P) for P in Ps) + bytes(64) + _g1b(bn.G1_GEN)
    g2 = b"".join(_g2b(Qg) for Qg in Qs) + _g2b(bn.G2_GEN) + bytes(128)
    n = len(g1) // 64  # 7 pairs: the lane kernels' last wavefront is partly filled
    one = T.gt_bytes(T.F12_ONE)
    ml_l, gt_l = gpu_ctx.pairing(g1, g2, final_exp=False), gpu_ctx.pairing(g1, g2)
    ml_w, gt_w = gpu_ctx.wave_pairing(g1, g2, final_exp=False), gpu_ctx.wave_pairing(g1, g2)
    for i in range(n):
        assert ml_w[384 * i:384 * i + 384] == ml_l[384 * i:384 * i + 384], i
        assert gt_w[384 * i:384 * i + 384] == gt_l[384 * i:384 * i + 384], i
    for i in (0, 1):  # the Python tower is slow
        f = T.miller_loop([(Ps[i], T.from_bn254_g2(Qs[i]))])
        assert ml_w[384 * i:384 * i + 384] == T.gt_bytes(f), i
        assert gt_w[384 * i:384 * i + 384] == T.gt_bytes(T.final_exp(f)), i
    assert gt_w[384 * 5:384 * 6] == one and gt_w[384 * 6:] == one  # (inf, G2), (G1, inf)
    # n = 1
    assert gpu_ctx.wave_pairing(g1[64:128], g2[128:256]) == gt_l[384:768]
    assert gpu_ctx.wave_pairing(g1[64:128], g2[128:256], final_exp=False) == ml_l[384:768]
    assert gpu_ctx.wave_pairing(b"", b"") == b""


def test_wave_pairing_invalid_points(gpu_ctx, outside_g2):
    from zkfl import native
    with pytest.raises(native.ZkflError) as e:  # off-curve G1
        gpu_ctx.wave_pairing(_le(1) + _le(3), _g2b(bn.G2_GEN))
    assert e.value.code == -1
    with pytest.raises(native.ZkflError) as e:  # on the twist, outside G2
        gpu_ctx.wave_pairing(_g1b(bn.G1_GEN) * 2, _g2b(bn.G2_GEN) + outside_g2)
    assert e.value.code == -1


# ---------------------------------------------------------------------------
# 2. round verdicts, two keys
# ---------------------------------------------------------------------------
def _setup_and_prove(ctx, b, inputs, toxic):
    from zkfl import groth16, native, zkey
    zk = zkey.groth16_setup(b, ctx, zkey.Toxic(**toxic))
    key = native.ProvingKey(ctx, zk)
    proof, pub = key.prove(zkey.wtns_bytes(ow.evaluate(b, inputs)))
    key.close()
    vkj = groth16.export_verification_key(zk, alphabeta=False)
    return zk, vkj, proof, list(pub)


KINDS = ("valid", "pub+1", "pub+r", "neg_a", "c+g", "a=(1,5)", "coord+q", "b_outside", "a_zero")


def _tamper(kind, proof, pub, outside):
    pub = list(pub)
    if kind == "pub+1":
        pub[-1] = (pub[-1] + 1) % R
    elif kind == "pub+r":
        pub[0] = pub[0] + R
        assert pub[0] < 1 << 256
    elif kind == "neg_a":
        proof = _g1b(bn.neg(bn.g1_from_bytes_std(proof[:64]))) + proof[64:]
    elif kind == "c+g":
        proof = proof[:192] + _g1b(bn.add(bn.g1_from_bytes_std(proof[192:]), bn.G1_GEN))
    elif kind == "a=(1,5)":
        proof = _le(1) + _le(5) + proof[64:]
    elif kind == "coord+q":
        proof = _le(int.from_bytes(proof[:32], "little") + Q) + proof[32:]
    elif kind == "b_outside":
        proof = proof[:64] + outside + proof[192:]
    elif kind == "a_zero":
        proof = bytes(64) + proof[64:]
    return proof, pub


@pytest.fixture(scope="module")
def round_jobs(gpu_ctx, outside_g2):
    """Two resident keys and 16 jobs alternating between them, cycling through the tamper kinds."""
    from zkfl import circuits, clients, groth16, native
    inp, _ = clients.Client(1, 8, 4, 3, clients.JsLcg(12345)).training_input(8, 1000, 100000000)
    made = [
        _setup_and_prove(gpu_ctx, circuits.build("poseidon_hash2"), {"left": 3, "right": 4},
                         dict(tau=4242, alpha=9, beta=10, gamma=11, delta=12)),
        _setup_and_prove(gpu_ctx, circuits.build("sgd_verified", 8, 4, 3, 1000), inp,
                         dict(tau=777, alpha=5, beta=6, gamma=7, delta=8)),
    ]
    assert [len(m[3]) for m in made] == [1, 6]
    keys = [native.VerifyingKey(gpu_ctx, groth16.vk_bytes(m[1])) for m in made]
    assert [k.n_public for k in keys] == [1, 6]
    jobs, want, meta = [], [], []
    for i in range(16):
        which, kind = i % 2, KINDS[(i // 2 + 5 * (i % 2)) % len(KINDS)]
        proof, pub = _tamper(kind, made[which][2], made[which][3], outside_g2)
        jobs.append((keys[which], b"".join(_le(x) for x in pub), proof))
        want.append(kind == "valid")
        meta.append((which, kind, pub))
    # both keys see every kind at least once over the 16 jobs, or at least both verdicts
    for which in (0, 1):
        assert {w for w, m in zip(want, meta) if m[0] == which} == {True, False}
    yield {"jobs": jobs, "want": want, "meta": meta, "made": made, "keys": keys}
    for k in keys:
        k.close()


def test_round_verdicts_two_keys(gpu_ctx, round_jobs):
    jobs, want, meta, made = (round_jobs[k] for k in ("jobs", "want", "meta", "made"))
    assert {m[1] for m in meta} == set(KINDS)
    got_w = gpu_ctx.verify_multi(jobs, "waves")
    got_l = gpu_ctx.verify_multi(jobs, "lanes")
    got_a = gpu_ctx.verify_multi(jobs, "auto")
    print("waves", got_w, "\nlanes", got_l, "\nwant ", want)
    assert got_w == want
    assert got_l == want
    assert got_a == want
    # the oracle agrees on one valid and one invalid job per key (in-range encodings only)
    for which in (0, 1):
        z = og.parse_zkey(made[which][0])
        idx = [i for i, m in enumerate(meta) if m[0] == which]
        pick = [next(i for i in idx if want[i]),
                next(i for i in idx if meta[i][1] in ("pub+1", "neg_a", "c+g"))]
        for i in pick:
            p = jobs[i][2]
            assert og.verify(z, meta[i][2], bn.g1_from_bytes_std(p[:64]), bn.g2_from_bytes_std(p[64:192]),
                             bn.g1_from_bytes_std(p[192:])) == want[i], i
    # another order: the same verdicts, permuted
    perm = list(range(16))
    random.Random(2).shuffle(perm)
    for sched in ("waves", "lanes"):
        assert gpu_ctx.verify_multi([jobs[i] for i in perm], sched) == [want[i] for i in perm], sched


# ---------------------------------------------------------------------------
# 3. vk_x digits
# ---------------------------------------------------------------------------
def test_vk_x_window_digits(gpu_ctx):
    """x_i * y = z_i with four public x_i: valid proofs for freely chosen public signals, so the
    per-window tables meet digit 0 and digit 15 in every position with a proof that must pass."""
    from zkfl import groth16, native, zkey
    from zkfl.r1cs import Builder
    b = Builder("pub_digits")
    xs = b.input("x", (4,), public=True)
    y = b.input("y")
    for x in xs:
        b.mul(x, y)
    zk = zkey.groth16_setup(b, gpu_ctx, zkey.Toxic(tau=991, alpha=2, beta=3, gamma=5, delta=7))
    pk = native.ProvingKey(gpu_ctx, zk)
    vk = native.VerifyingKey(gpu_ctx, groth16.vk_bytes(groth16.export_verification_key(zk, alphabeta=False)))
    assert vk.n_public == 4
    lo = int("0f" * 32, 16)
    hi = int("20" + "f0" * 31, 16)  # 0xF0...F0 with the top byte cut to stay < r (r = 0x3064...)
    jobs, want = [], []
    for pubs in ((0, 1, R - 1, lo), (R - 1, R - 1, 0, hi)):
        assert all(0 <= p < R for p in pubs)
        proof, pub = pk.prove(zkey.wtns_bytes(ow.evaluate(b, {"x": list(pubs), "y": 12345})))
        assert tuple(pub) == pubs
        jobs.append((vk, b"".join(_le(p) for p in pubs), proof))
        want.append(True)
        for j in range(4):
            for d in (1, -1):
                t = list(pubs)
                t[j] = (t[j] + d) % R
                jobs.append((vk, b"".join(_le(p) for p in t), proof))
                want.append(False)
    got_w = gpu_ctx.verify_multi(jobs, "waves")
    got_l = gpu_ctx.verify_multi(jobs, "lanes")
    print("waves", got_w, "\nlanes", got_l)
    assert got_w == want
    assert got_l == want
    pk.close()
    vk.close()


# ---------------------------------------------------------------------------
# 4. key objects
# ---------------------------------------------------------------------------
def test_key_objects_and_errors(gpu_ctx, round_jobs):
    import ctypes as C
    from zkfl import circuits, groth16, native
    jobs, want, made, keys = (round_jobs[k] for k in ("jobs", "want", "made", "keys"))
    # a third key through the context's one-slot cache, interleaved with the resident two
    zk3, vkj3, proof3, pub3 = _setup_and_prove(gpu_ctx, circuits.build("poseidon_hash2"), {"left": 8, "right": 9},
                                               dict(tau=31337, alpha=4, beta=6, gamma=8, delta=10))
    vk3, pubb3 = groth16.vk_bytes(vkj3), b"".join(_le(x) for x in pub3)
    for sched in ("waves", "lanes"):
        assert gpu_ctx.verify(vk3, pubb3, proof3) is True
        assert gpu_ctx.verify_multi(jobs[:4], sched) == want[:4]
        assert gpu_ctx.verify(vk3, _le(pub3[0] + 1), proof3) is False
        assert gpu_ctx.verify(vk3, pubb3, proof3) is True
    # the third key's proof does not verify under the first resident key (same circuit, other ceremony)
    assert gpu_ctx.verify_multi([(keys[0], pubb3, proof3)], "waves") == [False]
    # malformed images
    vk0 = groth16.vk_bytes(made[0][1])
    with pytest.raises(native.ZkflError) as e:
        native.VerifyingKey(gpu_ctx, vk0[:-10])
    assert e.value.code == -2
    bad = bytearray(vk0)
    bad[4:36] = _le(12345)  # alpha1 off curve
    with pytest.raises(native.ZkflError) as e:
        native.VerifyingKey(gpu_ctx, bytes(bad))
    assert e.value.code == -2
    # npubs off by one: ZKFL_E_MISMATCH naming the job, results untouched
    L = native.lib()
    n = 3
    hk = (C.c_void_p * n)(*[jobs[i][0].h for i in range(n)])
    pubs = (C.c_char_p * n)(*[jobs[i][1] for i in range(n)])
    npubs = (C.c_size_t * n)(*[len(jobs[i][1]) // 32 for i in range(n)])
    npubs[1] += 1
    res = (C.c_int32 * n)(7, 7, 7)
    proofs = b"".join(jobs[i][2] for i in range(n))
    assert L.zkfl_groth16_verify_multi(gpu_ctx.h, n, hk, pubs, npubs, proofs, res, 2) == -4
    assert "job 1" in L.zkfl_last_error().decode()
    assert list(res) == [7, 7, 7]
    npubs[1] -= 1
    assert L.zkfl_groth16_verify_multi(gpu_ctx.h, n, hk, pubs, npubs, proofs, res, 5) == -1  # unknown schedule
    assert list(res) == [7, 7, 7]
    assert L.zkfl_groth16_verify_multi(gpu_ctx.h, 0, None, None, None, None, None, 0) == 0
    assert gpu_ctx.verify_multi([]) == []
    assert L.zkfl_groth16_verify_multi(gpu_ctx.h, n, hk, pubs, npubs, proofs, res, 2) == 0
    assert [bool(x) for x in res] == want[:3]
    # a key above the wave-table cap: a valid key padded with infinite IC points, zero publics
    src = open(os.path.join(ROOT, "include", "zkfl.h")).read()
    import re
    cap = int(re.search(r"#define\s+ZKFL_VERIFY_WAVE_MAX_PUBLIC\s+(\d+)", src).group(1))
    extra = cap + 1 - 1  # nPublic 1 -> cap + 1
    big = (cap + 1).to_bytes(4, "little") + vk0[4:] + bytes(64 * extra)
    kbig = native.VerifyingKey(gpu_ctx, big)
    assert kbig.n_public == cap + 1
    pub_ok = jobs[0][1] + bytes(32 * extra)
    pub_bad = _le(made[0][3][0] + 1) + bytes(32 * extra)
    assert want[0] is True
    mixed = [(kbig, pub_ok, jobs[0][2]), jobs[0], (kbig, pub_bad, jobs[0][2]), jobs[1]]
    for sched in ("waves", "auto", "lanes"):
        assert gpu_ctx.verify_multi(mixed, sched) == [True, True, False, want[1]], sched
    kbig.close()


# ---------------------------------------------------------------------------
# 5. CLI
# ---------------------------------------------------------------------------
def test_cli_verify_round(gpu_ctx, round_jobs, tmp_path):
    from zkfl import groth16, native
    jobs, want, meta, made = (round_jobs[k] for k in ("jobs", "want", "meta", "made"))
    for which in (0, 1):
        (tmp_path / f"vkey{which}.json").write_text(json.dumps(made[which][1]))
    # in-range public signals only (public.json holds decimal strings of any size, but keep it plain)
    sel = [i for i in range(16) if meta[i][1] in ("valid", "pub+1", "neg_a", "c+g")]
    entries = {}
    for i in sel:
        (tmp_path / f"public{i}.json").write_text(json.dumps([str(x) for x in meta[i][2]]))
        (tmp_path / f"proof{i}.json").write_text(json.dumps(groth16.proof_to_json(jobs[i][2])))
        entries[i] = {"vkey": f"vkey{meta[i][0]}.json", "public": f"public{i}.json", "proof": f"proof{i}.json"}
    valid = [i for i in sel if want[i]]
    assert {meta[i][0] for i in valid} == {0, 1} and len(sel) > len(valid)
    (tmp_path / "good.json").write_text(json.dumps([entries[i] for i in valid]))
    (tmp_path / "mixed.json").write_text(json.dumps([entries[i] for i in sel]))
    env = dict(os.environ, PYTHONPATH=os.path.dirname(native.LIB_PATH) + os.pathsep + ROOT)

    def run(name):
        return subprocess.run([sys.executable, "-m", "zkfl", "verify-round", name], cwd=tmp_path, env=env,
                              capture_output=True, text=True, timeout=300)

    ok = run("good.json")
    assert ok.returncode == 0, ok.stderr
    assert ok.stdout.splitlines() == [f"job {j}: [INFO]  snarkJS: OK!" for j in range(len(valid))]
    mixed = run("mixed.json")
    assert mixed.returncode == 1, mixed.stderr
    assert mixed.stdout.splitlines() == [
        f"job {j}: " + ("[INFO]  snarkJS: OK!" if want[i] else "[ERROR] snarkJS: Invalid proof")
        for j, i in enumerate(sel)]
