"""`zkey check` without a GPU: the CPU model (tests/keycheck_model.py) on honest and tampered keys of
tiny_circuit() over a power-4 ptau built on the oracle's point backend, and the command line's
argument handling.

The model is the reference tests/test_gpu_keycheck.py holds the GPU to; the tamper table
(tests/keycheck_tampers.py) is what keeps a check from being vacuous: each tamper must fail exactly
its checks, and every check has a tamper that only it catches.
"""
import os
import random
import subprocess
import sys
import types

import pytest

import keycheck_model as model
import keycheck_tampers as tp
from oracle_backend import OraclePoints
from test_ptau_cpu import ALPHA, BETA, TAU, tiny_circuit
from zkfl import ptau, zkey
from zkfl.field import R

D1, D2 = 0x5555, 0x1F2E3D


@pytest.fixture(scope="module")
def world():
    be = OraclePoints()
    b = tiny_circuit()
    p2 = ptau.prepare_phase2(ptau.contribute(ptau.new(4), be, TAU, ALPHA, BETA), be)
    zk0 = zkey.setup_from_ptau(b, p2, be)
    zk1 = zkey.zkey_contribute(zk0, be, D1)
    zk2 = zkey.zkey_contribute(zk1, be, D2)
    dev = zkey.groth16_setup(b, be, zkey.Toxic(tau=TAU, alpha=ALPHA, beta=BETA, gamma=7, delta=11))
    rng = random.Random(20240607)
    n = zkey.domain_size_for(b)
    rho = [rng.randrange(R) for _ in range(b.n_wires)]
    sigma = [rng.randrange(R) for _ in range(n)]

    def check(zk, pt=p2, cons=None):
        return model.check(b.cons if cons is None else cons, b.n_wires, b.n_public, pt, zk, rho, sigma)
    return types.SimpleNamespace(be=be, b=b, ptau=p2, keys=dict(delta1=zk0, one=zk1, two=zk2, dev=dev), check=check)


ALL_PASS = {c: "pass" for c in model.CHECKS}


@pytest.mark.parametrize("which", ["delta1", "one", "two", "dev"])
def test_honest_keys_pass(world, which):
    """delta = 1, one and two contributions, and the dev ceremony's key with the ptau's tau, alpha,
    beta and gamma = 7, delta = 11."""
    out = world.check(world.keys[which])
    assert out["checks"] == ALL_PASS and out["first_failed"] is None


@pytest.mark.parametrize("name", sorted(tp.TAMPERS))
def test_tamper_fails_exactly_its_checks(world, name):
    out = world.check(tp.TAMPERS[name][0](world.keys["one"]))
    assert out["checks"] == tp.expected(name), name


def test_every_check_has_a_tamper_only_it_catches():
    alone = {next(iter(f)) for _, f, _ in tp.TAMPERS.values() if len(f) == 1}
    assert alone == set(model.CHECKS)


def test_reports_name_section_index_and_row(world):
    zk = world.keys["one"]
    i = tp.live(zk, 5)[-1]
    out = world.check(tp.off_curve(tp.off_curve(zk, 5, i), 5, tp.live(zk, 5)[0]))
    assert out["point"] == (5, tp.live(zk, 5)[0], 2)
    out = world.check(tp.coef_plus_one(zk, 0))
    assert out["coef"] == (0, 0, 1)
    out = world.check(tp.term_moved(zk, 0))
    assert out["coef"] == (0, 0, 2)


def test_key_of_another_system(world):
    """The same system with one A coefficient changed (constraint 0, a private wire): section 4, A and
    that wire's C point differ; B1, B2, IC and H do not."""
    cons = [tuple(dict(m) for m in con) for con in world.b.cons]   # x * x shares one dict for A and B
    A = cons[0][0]
    w = next(iter(A))
    assert w > world.b.n_public
    A[w] = (A[w] + 1) % R
    other = types.SimpleNamespace(cons=cons, n_wires=world.b.n_wires, n_public=world.b.n_public,
                                  n_constraints=world.b.n_constraints)
    zk = zkey.zkey_contribute(zkey.setup_from_ptau(other, world.ptau, world.be), world.be, D1)
    out = world.check(zk)
    want = dict(ALL_PASS, coefficients="fail", A="fail", C="fail")
    assert out["checks"] == want
    assert world.check(zk, cons=cons)["checks"] == ALL_PASS


def test_ptau_of_another_tau(world):
    """The right key against a ptau with the same alpha and beta but another tau: the header holds,
    every query fails."""
    other = ptau.prepare_phase2(ptau.contribute(ptau.new(4), world.be, TAU + 1, ALPHA, BETA), world.be)
    out = world.check(world.keys["one"], pt=other)
    assert out["checks"] == dict(ALL_PASS, A="fail", B1="fail", B2="fail", IC="fail", C="fail", H="fail")


def test_header_counts(world):
    zk = world.keys["one"]
    o = tp.zsecs(zk)[2][0] + 76
    bad = tp.patch(zk, o, (world.b.n_public + 1).to_bytes(4, "little"))
    assert world.check(bad)["first_failed"] == "header"


def test_block_selection_is_shared(world):
    """setup_from_ptau and the check take their blocks from one function."""
    blk = zkey.ptau_blocks(world.b, world.ptau)
    pt = ptau.Ptau(world.ptau)
    assert blk["power"] == 3 and blk["n"] == 8
    assert blk["L"] == pt.lagrange(12, 3) and blk["L2"] == pt.lagrange(13, 3)
    assert blk["La"] == pt.lagrange(14, 3) and blk["Lb"] == pt.lagrange(15, 3)
    top = pt.lagrange(12, 4)
    assert blk["H0"] == b"".join(top[64 * (2 * j + 1):64 * (2 * j + 2)] for j in range(8))
    with pytest.raises(ValueError, match="not prepared"):
        zkey.ptau_blocks(world.b, ptau.new(4))


def _cli(*argv):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(zkey.__file__)))
    env = dict(os.environ, PYTHONPATH=pkg + os.pathsep + root)
    return subprocess.run([sys.executable, "-m", "zkfl", *argv], env=env, capture_output=True, text=True, timeout=120)


def test_cli_unusable_arguments_exit_2(world, tmp_path):
    """Wrong argument counts, missing files, an unprepared ptau and a file that is no .r1cs are
    decided before the GPU is touched: exit status 2."""
    r1, pt, zk = tmp_path / "c.r1cs", tmp_path / "pot.ptau", tmp_path / "c.zkey"
    r1.write_bytes(world.b.r1cs_bytes())
    pt.write_bytes(ptau.new(4))           # not prepared
    zk.write_bytes(world.keys["one"])
    assert _cli("zkey", "check").returncode == 2
    assert _cli("zkey", "check", str(r1), str(pt)).returncode == 2
    assert _cli("zkey", "check", str(r1), str(pt), str(zk), "extra").returncode == 2
    assert _cli("zkey", "check", str(r1), str(tmp_path / "none.ptau"), str(zk)).returncode == 2
    p = _cli("zkey", "check", str(r1), str(pt), str(zk))
    assert p.returncode == 2 and "not prepared" in p.stderr
    assert _cli("zkey", "check", str(zk), str(pt), str(zk)).returncode == 2
    # `zkey verify` asserts a contribution transcript, which the check does not test: unserved
    assert _cli("zkey", "verify", str(r1), str(pt), str(zk)).returncode == 99
