"""A failed round narrowed to its bad groups (zkfl_groth16_verify_round_narrow,
csrc/verify_round.hip) — MI355X.

Bar: with a caller's z every group's final-exponentiated value is, byte for byte, the product of
its unscreened jobs' check values raised to z_i as oracle/pairing_tower.py computes them
(tests/narrow_model.py) — through a key border inside a group, a short group, an infinite pi_a,
a C sum that passes through infinity, a group of screened jobs only and several passes; verdicts
equal verify_multi's "lanes" verdicts, and the report counts exactly the groups that fail and the
jobs re-verified, so an implementation that re-verifies everything does not pass.
"""
import ctypes as C
import json
import os
import random
import subprocess
import sys

import pytest

from oracle import bn254 as bn

import narrow_model as N
import verify_round_model as M
from test_gpu_verify_round import KINDS, SCREENED_KINDS, Z_MAX, Round, _g1b, _tamper

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rnd(gpu_ctx):
    r = Round(gpu_ctx)
    yield r
    r.close()


def _interleave(key0, key1):
    """Two lists of equal length (or key0 one longer) -> job order 0 1 0 1 ..: the call sorts them back."""
    out = []
    for i in range(len(key0)):
        out.append(key0[i])
        if i < len(key1):
            out.append(key1[i])
    return out


def _check_groups(ctx, pairs, zs, screened, chunk, group):
    jobs, model = [p[0] for p in pairs], [p[1] for p in pairs]
    group_of, values, scr = ctx.debug_verify_round_groups(jobs, zs, chunk, group)
    assert scr == screened
    want_of, want = N.expected_groups(model, zs, screened, chunk, group)
    assert group_of == want_of
    assert len(values) == len(want)
    for g, (got, exp) in enumerate(zip(values, want)):
        assert got == exp, f"group {g} (chunk {chunk}, group {group})"
    return group_of, values


# ---------------------------------------------------------------------------
# 1. every group's 384 B against the model
# ---------------------------------------------------------------------------
def test_group_parity_with_the_model(gpu_ctx, rnd):
    rng = random.Random(11)
    proof, pub = rnd.made[0][2], rnd.made[0][3]
    neg_c = rnd.custom(0, pub, proof[:192] + _g1b(bn.neg(bn.g1_from_bytes_std(proof[192:]))))
    # in the call's order (key 0's eleven jobs, then key 1's), groups of 4:
    #   0-3   pi_c and -pi_c next to each other with equal z (the C sum passes through infinity), pi_a = O
    #   4-7   screened jobs only
    #   8-11  three jobs of key 0 and one of key 1: two key segments
    #   16-19 valid jobs only; 20-21 the short group
    key0 = [rnd.job(0), neg_c, rnd.job(0, "a_zero"), rnd.job(0, "c+g")] + \
           [rnd.job(0, k) for k in SCREENED_KINDS] + [rnd.job(0, "pub+1"), rnd.job(0, "neg_a"), rnd.job(0)]
    key1 = [rnd.job(1, "neg_a")] + [rnd.job(1, k) for k in ("valid", "pub+1", "c+g", "valid")] + \
           [rnd.job(1)] * 4 + [rnd.job(1, "c+g"), rnd.job(1)]
    assert len(key0) == 11 and len(key1) == 11
    pairs = _interleave(key0, key1)
    zs = [rng.randrange(1 << 128) for _ in range(22)]
    zs[2] = zs[0]                      # neg_c is job 2, its partner job 0
    zs[8], zs[21] = 1, Z_MAX
    screened = [i % 2 == 0 and 4 <= i // 2 < 8 for i in range(22)]
    for chunk in (0, 10):
        group_of, values = _check_groups(gpu_ctx, pairs, zs, screened, chunk, 4)
        assert group_of[0] == group_of[2] == group_of[4] == 0          # pi_c, -pi_c, pi_a = O
        assert {group_of[i] for i in range(8, 16, 2)} == {1} and values[1] == M.GT_ONE  # screened only
        assert values[0] != M.GT_ONE
        assert group_of[20] == group_of[1]                               # a group with both keys
    group_of, values = _check_groups(gpu_ctx, pairs, zs, screened, 0, 4)
    assert len(values) == 6 and group_of.count(5) == 2                   # the short group
    assert values[4] == M.GT_ONE and values[5] != M.GT_ONE
    assert len(_check_groups(gpu_ctx, pairs, zs, screened, 10, 4)[1]) == 3 + 3 + 1
    # n = 1 and group = 1: each value is the job's own check value to the power z
    bad = rnd.job(1, "c+g")
    assert _check_groups(gpu_ctx, [bad], [1], [False], 0, 1)[1] == [M.T.gt_bytes(M.job_value(*bad[1]))]
    some = [rnd.job(0, "pub+1"), bad, rnd.job(0), rnd.job(1, "neg_a")]
    z4 = [rng.randrange(1 << 128), 1, Z_MAX, 0]
    group_of, values = _check_groups(gpu_ctx, some, z4, [False] * 4, 0, 1)
    assert group_of == [0, 2, 1, 3]
    assert values[2] == M.T.gt_bytes(M.job_value(*bad[1])) and values[1] == M.GT_ONE and values[3] == M.GT_ONE
    # group 0 in the hook: the production size, here one group for the whole pass
    assert gpu_ctx.debug_verify_round_groups([p[0] for p in some], z4)[0] == [0] * 4
    # the all-valid round: every group is the identity
    valid = _interleave([rnd.job(0)] * 11, [rnd.job(1)] * 11)
    for chunk in (0, 10):
        _, values, _ = gpu_ctx.debug_verify_round_groups([p[0] for p in valid], zs, chunk, 4)
        assert values == [M.GT_ONE] * len(values) and len(values) == (6 if chunk == 0 else 7)


# ---------------------------------------------------------------------------
# 2. only the bad groups' jobs are verified again
# ---------------------------------------------------------------------------
def test_narrowing_happens(gpu_ctx, rnd):
    kinds = ["valid"] * 32
    kinds[5], kinds[12] = "c+g", "pub+1"   # key 1's third job: group 4; key 0's seventh: group 1
    jobs = [rnd.job(i % 2, k)[0] for i, k in enumerate(kinds)]
    want = [k == "valid" for k in kinds]
    model = N.expected_report([i % 2 for i in range(32)], [False] * 32, want, 0, 4)
    assert (model["groups"], model["bad_groups"], model["fallback"]) == (8, 2, 8)
    got, rep = gpu_ctx.verify_round_narrow(jobs, None, 4)
    print(rep)
    assert got == want
    assert got == gpu_ctx.verify_multi(jobs, "lanes")
    assert rep == {"keys": 2, "screened": 0, "combined": 32, "passed": 0, "groups": 8, "bad_groups": 2, "fallback": 8}
    # the existing entry on the same jobs re-verifies them all
    assert gpu_ctx.verify_round(jobs)[1]["fallback"] == 32


# ---------------------------------------------------------------------------
# 3. verdicts and the report over the tamper kinds
# ---------------------------------------------------------------------------
def test_verdicts_and_report(gpu_ctx, rnd):
    kinds = [KINDS[(i // 2 + 5 * (i % 2)) % len(KINDS)] for i in range(16)]
    assert set(kinds) == set(KINDS)
    jobs = [rnd.job(i % 2, k)[0] for i, k in enumerate(kinds)]
    key_ids = [i % 2 for i in range(16)]
    want = [k == "valid" for k in kinds]
    scr = [k in SCREENED_KINDS for k in kinds]
    model = dict(N.expected_report(key_ids, scr, want, 0, 4), keys=2)
    assert model["bad_groups"] >= 2 and 0 < model["screened"] < 16
    got, rep = gpu_ctx.verify_round_narrow(jobs, None, 4)
    print(got, rep)
    assert got == want
    assert got == gpu_ctx.verify_multi(jobs, "lanes")
    assert rep == model
    # valid and screened only: the round passes, no group is looked at, nothing is re-verified
    keep = [i for i, k in enumerate(kinds) if k == "valid" or k in SCREENED_KINDS]
    got, rep = gpu_ctx.verify_round_narrow([jobs[i] for i in keep], None, 4)
    assert got == [want[i] for i in keep]
    assert (rep["passed"], rep["bad_groups"], rep["fallback"], rep["screened"]) == (1, 0, 0, sum(scr))
    # another order: the same verdicts, permuted, and the model's counts for that order
    perm = list(range(16))
    random.Random(4).shuffle(perm)
    got, rep = gpu_ctx.verify_round_narrow([jobs[i] for i in perm], None, 4)
    assert got == [want[i] for i in perm]
    assert rep == dict(N.expected_report([key_ids[i] for i in perm], [scr[i] for i in perm],
                                         [want[i] for i in perm], 0, 4), keys=2)
    # fresh z on every call: the same verdicts and report
    assert gpu_ctx.verify_round_narrow(jobs, None, 4) == (want, model)
    assert gpu_ctx.verify_round_narrow(jobs, None, 4) == (want, model)
    # a caller's z through the production entry
    assert gpu_ctx.verify_round_narrow(jobs, [Z_MAX] * 16, 4) == (want, model)


# ---------------------------------------------------------------------------
# 4. group = 0: the production policy
# ---------------------------------------------------------------------------
def test_policy(gpu_ctx, rnd):
    from zkfl import native
    NMIN, GROUP = native.ROUND_NARROW_MIN, native.ROUND_GROUP
    good, bad = [rnd.job(0)[0], rnd.job(1)[0]], rnd.job(1, "c+g")[0]
    if NMIN > 1:  # a round too small to narrow: zkfl_groth16_verify_round's behaviour
        n = NMIN - 1
        jobs = [good[i % 2] for i in range(n - 1)] + [bad]
        got, rep = gpu_ctx.verify_round_narrow(jobs)
        assert got == [True] * (n - 1) + [False]
        assert rep == {"keys": min(2, n), "screened": 0, "combined": n, "passed": 0, "groups": 0, "bad_groups": 0,
                       "fallback": n}
    m = max(NMIN, 70)
    jobs = [good[i % 2] for i in range(m - 1)] + [bad]
    got, rep = gpu_ctx.verify_round_narrow(jobs)
    print(rep)
    assert got == [True] * (m - 1) + [False]
    passes = [min(4096, m - off) for off in range(0, m, 4096)]
    assert rep["groups"] == sum(-(-p // GROUP) for p in passes)
    model = N.expected_report([i % 2 for i in range(m - 1)] + [1], [False] * m, got)
    assert rep == dict(model, keys=2)
    assert rep["bad_groups"] == 1 and rep["fallback"] < m


# ---------------------------------------------------------------------------
# 5. the production pass size: groups end at the pass border
# ---------------------------------------------------------------------------
def test_production_pass_border(gpu_ctx, rnd):
    n = 4096 + 70
    n0 = (n + 1) // 2  # key 0's jobs come first in the call's order: position p is job 2p, n0 + p is job 2p + 1
    kinds = ["valid"] * n
    bad_pos = (5, 4090, 4096 + 66)  # the first group; the last group of pass 1; pass 2's short group (6 jobs)
    for p in bad_pos:
        kinds[2 * p if p < n0 else 2 * (p - n0) + 1] = "c+g"
    made = {(w, k): rnd.job(w, k)[0] for w in (0, 1) for k in ("valid", "c+g")}
    jobs = [made[(i % 2, k)] for i, k in enumerate(kinds)]
    want = [k == "valid" for k in kinds]
    model = N.expected_report([i % 2 for i in range(n)], [False] * n, want, 0, 64)
    assert (model["groups"], model["bad_groups"], model["fallback"]) == (64 + 2, 3, 64 + 64 + 6)
    got, rep = gpu_ctx.verify_round_narrow(jobs, None, 64)
    print(rep)
    assert got == want
    assert rep == dict(model, keys=2)


# ---------------------------------------------------------------------------
# 6. errors
# ---------------------------------------------------------------------------
def test_errors(gpu_ctx, rnd):
    from zkfl import native
    L = native.lib()
    jobs = [rnd.job(0)[0], rnd.job(1)[0], rnd.job(0, "c+g")[0]]
    n = 3
    hk = (C.c_void_p * n)(*[j[0].h for j in jobs])
    pubs = (C.c_char_p * n)(*[j[1] for j in jobs])
    npubs = (C.c_size_t * n)(*[len(j[1]) // 32 for j in jobs])
    proofs = b"".join(j[2] for j in jobs)
    res = (C.c_int32 * n)(7, 7, 7)
    rep = (C.c_uint32 * 7)(*[9] * 7)
    group_of = (C.c_uint32 * n)(7, 7, 7)
    scr = (C.c_int32 * n)(7, 7, 7)
    out = (C.c_uint8 * (384 * n))()
    ng = C.c_uint32(77)
    z = bytes(16 * n)
    # npubs off by one: ZKFL_E_MISMATCH naming the job, results untouched
    npubs[1] += 1
    assert L.zkfl_groth16_verify_round_narrow(gpu_ctx.h, n, hk, pubs, npubs, proofs, None, 2, res, rep) == -4
    assert "job 1" in L.zkfl_last_error().decode()
    assert list(res) == [7, 7, 7] and list(rep) == [9] * 7
    assert L.zkfl_debug_verify_round_groups(gpu_ctx.h, n, hk, pubs, npubs, proofs, z, 0, 2, group_of, out, n,
                                            C.byref(ng), scr) == -4
    assert list(group_of) == [7, 7, 7] and list(scr) == [7, 7, 7] and ng.value == 77
    npubs[1] -= 1
    # a group above the pass size
    assert L.zkfl_groth16_verify_round_narrow(gpu_ctx.h, n, hk, pubs, npubs, proofs, None, 4, res, rep) == -1
    assert "group" in L.zkfl_last_error().decode()
    assert list(res) == [7, 7, 7] and list(rep) == [9] * 7
    assert L.zkfl_debug_verify_round_groups(gpu_ctx.h, n, hk, pubs, npubs, proofs, z, 2, 3, group_of, out, n,
                                            C.byref(ng), scr) == -1  # passes of 2
    # the hook needs z
    assert L.zkfl_debug_verify_round_groups(gpu_ctx.h, n, hk, pubs, npubs, proofs, None, 0, 2, group_of, out, n,
                                            C.byref(ng), scr) == -1
    # too little room: the count needed, nothing else written
    assert L.zkfl_debug_verify_round_groups(gpu_ctx.h, n, hk, pubs, npubs, proofs, z, 0, 1, group_of, out, 2,
                                            C.byref(ng), scr) == -1
    assert ng.value == 3 and list(group_of) == [7, 7, 7] and bytes(out) == bytes(384 * n)
    assert L.zkfl_debug_verify_round_groups(gpu_ctx.h, n, hk, pubs, npubs, proofs, z, 0, 1, group_of, out, 3,
                                            C.byref(ng), scr) == 0
    assert ng.value == 3 and list(group_of) == [0, 2, 1] and list(scr) == [0, 0, 0]
    assert bytes(out) == M.GT_ONE * 3  # z = 0
    # the pass size itself is a legal group; no report
    assert L.zkfl_groth16_verify_round_narrow(gpu_ctx.h, n, hk, pubs, npubs, proofs, None, 3, res, None) == 0
    assert [bool(x) for x in res] == [True, True, False]
    # n = 0
    assert L.zkfl_groth16_verify_round_narrow(gpu_ctx.h, 0, None, None, None, None, None, 0, None, None) == 0
    assert gpu_ctx.verify_round_narrow([], None, 4) == ([], {"keys": 0, "screened": 0, "combined": 0, "passed": 1,
                                                             "groups": 0, "bad_groups": 0, "fallback": 0})
    assert L.zkfl_debug_verify_round_groups(gpu_ctx.h, 0, None, None, None, None, None, 0, 0, None, None, 0,
                                            C.byref(ng), None) == 0
    assert ng.value == 0


# ---------------------------------------------------------------------------
# 7. CLI
# ---------------------------------------------------------------------------
def test_cli_verify_round_narrow(gpu_ctx, rnd, tmp_path):
    from zkfl import groth16, native
    for which in (0, 1):
        (tmp_path / f"vkey{which}.json").write_text(json.dumps(rnd.made[which][1]))
    picks = [(0, "valid"), (1, "valid"), (0, "valid"), (1, "c+g"), (0, "valid"), (1, "valid")]
    entries = []
    for i, (which, kind) in enumerate(picks):
        proof, pub = _tamper(kind, rnd.made[which][2], rnd.made[which][3], rnd.outside)
        (tmp_path / f"public{i}.json").write_text(json.dumps([str(x) for x in pub]))
        (tmp_path / f"proof{i}.json").write_text(json.dumps(groth16.proof_to_json(proof)))
        entries.append({"vkey": f"vkey{which}.json", "public": f"public{i}.json", "proof": f"proof{i}.json"})
    (tmp_path / "round.json").write_text(json.dumps(entries))
    env = dict(os.environ, PYTHONPATH=os.path.dirname(native.LIB_PATH) + os.pathsep + ROOT)

    def run(flag):
        return subprocess.run([sys.executable, "-m", "zkfl", "verify-round", flag, "round.json"], cwd=tmp_path, env=env,
                              capture_output=True, text=True, timeout=300)

    comb, narrow = run("--combined"), run("--narrow")
    assert comb.returncode == 1, comb.stderr
    assert narrow.returncode == 1, narrow.stderr
    assert narrow.stdout == comb.stdout
    assert narrow.stdout.splitlines() == [
        f"job {j}: " + ("[INFO]  snarkJS: OK!" if kind == "valid" else "[ERROR] snarkJS: Invalid proof")
        for j, (_, kind) in enumerate(picks)]
    report = [ln for ln in narrow.stderr.splitlines() if "narrowed" in ln]
    assert len(report) == 1
    for word in ("keys 2", "passed 0", "groups", "bad_groups", "fallback"):
        assert word in report[0]
