"""A round verified as one random combination with one final exponentiation
(zkfl_groth16_verify_round, csrc/verify_round.hip) — MI355X.

Bar: with a caller's z the final-exponentiated combination is, byte for byte, the product of the
per-job check values raised to z_i as oracle/pairing_tower.py computes them
(tests/verify_round_model.py) — through P + P and P + (-P) in the per-key sums, a partly filled
wavefront and several passes; verdicts equal verify_multi's "lanes" verdicts and the expected list
per tamper kind, and the report counts what was screened, combined and re-verified.
"""
import ctypes as C
import json
import os
import random
import re
import subprocess
import sys

import pytest

from oracle import bn254 as bn
from oracle import groth16 as og
from oracle import witness as ow

import verify_round_model as M

pytestmark = pytest.mark.gpu

R, Q = bn.R, bn.Q
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z_MAX = (1 << 128) - 1


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
            if bn.mul(P, R - 1) != bn.neg(P):  # [r]P != O
                return P
        x += 1


def _le(x):
    return int(x).to_bytes(32, "little")


def _g1b(P):
    return bn.g1_to_bytes_std(P)


KINDS = ("valid", "pub+1", "pub+r", "neg_a", "c+g", "a=(1,5)", "coord+q", "b_outside", "a_zero")
SCREENED_KINDS = ("pub+r", "a=(1,5)", "coord+q", "b_outside")


def _tamper(kind, proof, pub, outside):  # tests/test_gpu_verify_multi.py's
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


def _setup_and_prove(ctx, b, inputs, toxic):
    from zkfl import groth16, native, zkey
    zk = zkey.groth16_setup(b, ctx, zkey.Toxic(**toxic))
    key = native.ProvingKey(ctx, zk)
    proof, pub = key.prove(zkey.wtns_bytes(ow.evaluate(b, inputs)))
    key.close()
    return zk, groth16.export_verification_key(zk, alphabeta=False), proof, list(pub)


class Round:
    """The two circuits of tests/test_gpu_verify_multi.py: resident keys, one valid proof each."""

    def __init__(self, ctx):
        from zkfl import circuits, clients, groth16, native
        inp, _ = clients.Client(1, 8, 4, 3, clients.JsLcg(12345)).training_input(8, 1000, 100000000)
        self.made = [
            _setup_and_prove(ctx, circuits.build("poseidon_hash2"), {"left": 3, "right": 4},
                             dict(tau=4242, alpha=9, beta=10, gamma=11, delta=12)),
            _setup_and_prove(ctx, circuits.build("sgd_verified", 8, 4, 3, 1000), inp,
                             dict(tau=777, alpha=5, beta=6, gamma=7, delta=8)),
        ]
        assert [len(m[3]) for m in self.made] == [1, 6]
        self.keys = [native.VerifyingKey(ctx, groth16.vk_bytes(m[1])) for m in self.made]
        self.vks = [og.parse_zkey(m[0]) for m in self.made]
        self.outside = bn.g2_to_bytes_std(_twist_point_outside_g2())

    def job(self, which, kind="valid"):
        """-> (the GPU's job, the model's job)"""
        proof, pub = _tamper(kind, self.made[which][2], self.made[which][3], self.outside)
        return self.custom(which, pub, proof)

    def custom(self, which, pub, proof):
        return (self.keys[which], b"".join(_le(x) for x in pub), proof), (self.vks[which], which, pub, proof)

    def close(self):
        for k in self.keys:
            k.close()


@pytest.fixture(scope="module")
def rnd(gpu_ctx):
    r = Round(gpu_ctx)
    yield r
    r.close()


def _split(pairs):
    return [p[0] for p in pairs], [p[1] for p in pairs]


def _check(ctx, pairs, zs, chunk=0):
    """debug_verify_round against the model; nothing screened."""
    jobs, model = _split(pairs)
    gt, screened = ctx.debug_verify_round(jobs, zs, chunk)
    assert screened == [False] * len(jobs)
    want = M.expected_gt(model, zs)
    assert gt == want
    return gt


# ---------------------------------------------------------------------------
# 1. GT parity with a caller's z
# ---------------------------------------------------------------------------
def test_gt_parity_with_the_model(gpu_ctx, rnd):
    rng = random.Random(1)
    kinds = ("valid", "pub+1", "neg_a", "c+g")
    plan = [(i % 2, kinds[(i // 2 + i) % 4]) for i in range(9)]  # interleaved keys
    assert set(plan) == {(w, k) for w in (0, 1) for k in kinds}  # every kind on both keys
    pairs = [rnd.job(w, k) for w, k in plan]
    zs = [0, 1, Z_MAX] + [rng.randrange(1 << 128) for _ in range(6)]
    gt = _check(gpu_ctx, pairs, zs)
    assert gt != M.GT_ONE
    # the valid jobs alone: the identity, whatever z
    valid = [rnd.job(0), rnd.job(1), rnd.job(0), rnd.job(1)]
    assert _check(gpu_ctx, valid, [Z_MAX, rng.randrange(1 << 128), 1, rng.randrange(1 << 128)]) == M.GT_ONE
    # n = 1: z = 1 gives the job's own check value
    bad = rnd.job(1, "c+g")
    assert _check(gpu_ctx, [bad], [1]) == M.T.gt_bytes(M.job_value(*bad[1]))
    _check(gpu_ctx, [bad], [Z_MAX])
    assert _check(gpu_ctx, [bad], [0]) == M.GT_ONE


# ---------------------------------------------------------------------------
# 2. the per-key sums through P + P, P + (-P) and an infinite pi_a
# ---------------------------------------------------------------------------
def test_exceptional_sums(gpu_ctx, rnd):
    z = random.Random(2).randrange(1 << 128)
    for which in (0, 1):
        # the same job twice, equal z: X_k and C_k (and z alpha) add a point to itself
        bad = rnd.job(which, "pub+1")
        _check(gpu_ctx, [bad, bad], [z, z])
        assert _check(gpu_ctx, [rnd.job(which)] * 2, [z, z]) == M.GT_ONE
        # pi_c = C and -C, equal z: C_k passes through infinity (and ends there)
        proof, pub = rnd.made[which][2], rnd.made[which][3]
        neg_c = proof[:192] + _g1b(bn.neg(bn.g1_from_bytes_std(proof[192:])))
        gt = _check(gpu_ctx, [rnd.job(which), rnd.custom(which, pub, neg_c)], [z, z])
        assert gt != M.GT_ONE
        # ... and with a third job behind them, so the sum leaves infinity again
        _check(gpu_ctx, [rnd.job(which), rnd.custom(which, pub, neg_c), rnd.job(which, "c+g")], [z, z, 5])
    # pi_a = O: the pair (pi_a, pi_b) contributes 1
    _check(gpu_ctx, [rnd.job(0, "a_zero")], [z])
    _check(gpu_ctx, [rnd.job(1), rnd.job(0, "a_zero"), rnd.job(1, "a_zero")], [3, z, Z_MAX])


# ---------------------------------------------------------------------------
# 3. a partly filled last wavefront; three passes
# ---------------------------------------------------------------------------
def test_trees_and_passes(gpu_ctx, rnd):
    rng = random.Random(3)
    four = [rnd.job(0), rnd.job(1, "neg_a"), rnd.job(0, "c+g"), rnd.job(1)]
    pairs = [four[rng.randrange(4)] for _ in range(70)]
    zs = [rng.randrange(1 << 128) for _ in range(70)]
    jobs, model = _split(pairs)
    want = M.expected_gt(model, zs)
    one_pass, scr = gpu_ctx.debug_verify_round(jobs, zs)
    assert scr == [False] * 70
    three_passes, scr = gpu_ctx.debug_verify_round(jobs, zs, 32)  # 32 + 32 + 6, keys cut by the pass borders
    assert scr == [False] * 70
    assert one_pass == want
    assert three_passes == want
    # all valid, several passes
    jobs = [four[0][0], four[3][0]] * 35
    assert gpu_ctx.debug_verify_round(jobs, zs, 32)[0] == M.GT_ONE
    assert gpu_ctx.debug_verify_round(jobs, zs, 1)[0] == M.GT_ONE  # one proof per pass


# ---------------------------------------------------------------------------
# 4. verdicts and the report
# ---------------------------------------------------------------------------
def test_verdicts_and_report(gpu_ctx, rnd):
    kinds = [KINDS[(i // 2 + 5 * (i % 2)) % len(KINDS)] for i in range(16)]
    assert set(kinds) == set(KINDS)
    jobs = [rnd.job(i % 2, k)[0] for i, k in enumerate(kinds)]
    want = [k == "valid" for k in kinds]
    n_scr = sum(k in SCREENED_KINDS for k in kinds)
    assert 0 < n_scr < 16 and any(want)
    got, rep = gpu_ctx.verify_round(jobs)
    print(got, rep)
    assert got == want
    assert got == gpu_ctx.verify_multi(jobs, "lanes")
    assert rep == {"keys": 2, "screened": n_scr, "combined": 16 - n_scr, "passed": 0, "fallback": 16 - n_scr}
    # which jobs were screened
    _, scr = gpu_ctx.debug_verify_round(jobs, [1] * 16)
    assert scr == [k in SCREENED_KINDS for k in kinds]
    # the valid jobs alone
    valid = [j for j, w in zip(jobs, want) if w]
    got, rep = gpu_ctx.verify_round(valid)
    assert got == [True] * len(valid)
    assert rep == {"keys": len({id(j[0]) for j in valid}), "screened": 0, "combined": len(valid), "passed": 1,
                   "fallback": 0}
    # valid and screened only: the combination passes, nothing is re-verified
    some = [j for j, k in zip(jobs, kinds) if k == "valid" or k in SCREENED_KINDS]
    got, rep = gpu_ctx.verify_round(some)
    assert got == [k == "valid" for k in kinds if k == "valid" or k in SCREENED_KINDS]
    assert (rep["passed"], rep["fallback"], rep["screened"]) == (1, 0, n_scr)
    # another order: the same verdicts, permuted
    perm = list(range(16))
    random.Random(4).shuffle(perm)
    assert gpu_ctx.verify_round([jobs[i] for i in perm])[0] == [want[i] for i in perm]
    # fresh z on every call: the same verdicts
    assert gpu_ctx.verify_round(jobs, None)[0] == want
    assert gpu_ctx.verify_round(jobs, None)[0] == want
    # a caller's z through the production entry
    got, rep = gpu_ctx.verify_round(jobs, [Z_MAX] * 16)
    assert got == want and rep["passed"] == 0


# ---------------------------------------------------------------------------
# 5. keys and errors
# ---------------------------------------------------------------------------
def test_keys_and_errors(gpu_ctx, rnd):
    from zkfl import groth16, native
    L = native.lib()
    src = open(os.path.join(ROOT, "include", "zkfl.h")).read()
    cap = int(re.search(r"#define\s+ZKFL_VERIFY_WAVE_MAX_PUBLIC\s+(\d+)", src).group(1))
    # a key above the wave-table cap: key 0 padded with infinite IC points, zero publics
    vk0 = groth16.vk_bytes(rnd.made[0][1])
    big = (cap + 1).to_bytes(4, "little") + vk0[4:] + bytes(64 * cap)
    kbig = native.VerifyingKey(gpu_ctx, big)
    assert kbig.n_public == cap + 1
    j0, m0 = rnd.job(0)
    j1, m1 = rnd.job(1, "pub+1")
    pub_ok = j0[1] + bytes(32 * cap)
    pub_bad = _le(rnd.made[0][3][0] + 1) + bytes(32 * cap)
    mixed = [(kbig, pub_ok, j0[2]), j0, (kbig, pub_bad, j0[2]), j1]
    got, rep = gpu_ctx.verify_round(mixed)
    assert got == [True, True, False, False]
    assert rep == {"keys": 3, "screened": 0, "combined": 4, "passed": 0, "fallback": 4}
    got, rep = gpu_ctx.verify_round(mixed[:2])
    assert got == [True, True] and rep["passed"] == 1 and rep["keys"] == 2
    # the padded key's vk_x is key 0's: the model's values are key 0's
    zs = [7, Z_MAX, 11, 13]
    bad0 = rnd.custom(0, [rnd.made[0][3][0] + 1], j0[2])[1]
    gt, scr = gpu_ctx.debug_verify_round(mixed, zs)
    assert scr == [False] * 4
    assert gt == M.expected_gt([m0, m0, bad0, m1], zs)
    kbig.close()
    # npubs off by one: ZKFL_E_MISMATCH naming the job, results untouched
    jobs = [rnd.job(0)[0], rnd.job(1)[0], rnd.job(0, "c+g")[0]]
    n = 3
    hk = (C.c_void_p * n)(*[j[0].h for j in jobs])
    pubs = (C.c_char_p * n)(*[j[1] for j in jobs])
    npubs = (C.c_size_t * n)(*[len(j[1]) // 32 for j in jobs])
    npubs[1] += 1
    res = (C.c_int32 * n)(7, 7, 7)
    rep = (C.c_uint32 * 5)(9, 9, 9, 9, 9)
    proofs = b"".join(j[2] for j in jobs)
    assert L.zkfl_groth16_verify_round(gpu_ctx.h, n, hk, pubs, npubs, proofs, None, res, rep) == -4
    assert "job 1" in L.zkfl_last_error().decode()
    assert list(res) == [7, 7, 7] and list(rep) == [9] * 5
    out = (C.c_uint8 * 384)()
    scr = (C.c_int32 * n)(7, 7, 7)
    assert L.zkfl_debug_verify_round(gpu_ctx.h, n, hk, pubs, npubs, proofs, bytes(16 * n), 0, out, scr) == -4
    assert "job 1" in L.zkfl_last_error().decode()
    assert list(scr) == [7, 7, 7]
    assert L.zkfl_debug_verify_round(gpu_ctx.h, n, hk, pubs, npubs, proofs, None, 0, out, scr) == -1  # z is required
    npubs[1] -= 1
    assert L.zkfl_groth16_verify_round(gpu_ctx.h, n, hk, pubs, npubs, proofs, None, res, None) == 0  # no report
    assert [bool(x) for x in res] == [True, True, False]
    # a key of another context
    with native.Context(0) as other:
        k2 = native.VerifyingKey(other, groth16.vk_bytes(rnd.made[0][1]))
        with pytest.raises(native.ZkflError) as e:
            gpu_ctx.verify_round([jobs[0], (k2, jobs[0][1], jobs[0][2])])
        assert e.value.code == -1 and "job 1" in str(e.value)
        k2.close()
    # n = 0
    assert L.zkfl_groth16_verify_round(gpu_ctx.h, 0, None, None, None, None, None, None, None) == 0
    assert gpu_ctx.verify_round([]) == ([], {"keys": 0, "screened": 0, "combined": 0, "passed": 1, "fallback": 0})
    assert L.zkfl_debug_verify_round(gpu_ctx.h, 0, None, None, None, None, None, 0, None, None) == 0


# ---------------------------------------------------------------------------
# 6. CLI
# ---------------------------------------------------------------------------
def test_cli_verify_round_combined(gpu_ctx, rnd, tmp_path):
    from zkfl import groth16, native
    for which in (0, 1):
        (tmp_path / f"vkey{which}.json").write_text(json.dumps(rnd.made[which][1]))
    picks = [(0, "valid"), (1, "valid"), (0, "pub+1"), (1, "neg_a"), (0, "c+g"), (1, "valid")]
    entries = []
    for i, (which, kind) in enumerate(picks):
        proof, pub = _tamper(kind, rnd.made[which][2], rnd.made[which][3], rnd.outside)
        (tmp_path / f"public{i}.json").write_text(json.dumps([str(x) for x in pub]))
        (tmp_path / f"proof{i}.json").write_text(json.dumps(groth16.proof_to_json(proof)))
        entries.append({"vkey": f"vkey{which}.json", "public": f"public{i}.json", "proof": f"proof{i}.json"})
    want = [k == "valid" for _, k in picks]
    (tmp_path / "good.json").write_text(json.dumps([e for e, w in zip(entries, want) if w]))
    (tmp_path / "mixed.json").write_text(json.dumps(entries))
    env = dict(os.environ, PYTHONPATH=os.path.dirname(native.LIB_PATH) + os.pathsep + ROOT)

    def run(name, *flags):
        return subprocess.run([sys.executable, "-m", "zkfl", "verify-round", *flags, name], cwd=tmp_path, env=env,
                              capture_output=True, text=True, timeout=300)

    for name, code, verdicts in (("good.json", 0, [True] * sum(want)), ("mixed.json", 1, want)):
        plain, comb = run(name), run(name, "--combined")
        assert plain.returncode == code, plain.stderr
        assert comb.returncode == code, comb.stderr
        assert comb.stdout == plain.stdout
        assert plain.stdout.splitlines() == [
            f"job {j}: " + ("[INFO]  snarkJS: OK!" if ok else "[ERROR] snarkJS: Invalid proof")
            for j, ok in enumerate(verdicts)]
        report = [ln for ln in comb.stderr.splitlines() if "combined round" in ln]
        assert len(report) == 1
        assert f"passed {1 if code == 0 else 0}" in report[0] and "keys 2" in report[0]
