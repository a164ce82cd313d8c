"""`zkey check` on the GPU (zkfl_zkey_check, csrc/keycheck.hip) -- MI355X.

Is a .zkey the Groth16 proving key of a .r1cs over a prepared .ptau, for some delta and gamma?  The
reference trusts any `<c>_final.zkey` it finds (tests/full_system_simulation.mjs:713-738).  Honest
keys of every setup path pass; the tamper table of tests/keycheck_tampers.py fails exactly its checks
(the contract tests/test_keycheck_cpu.py holds the CPU model to), with the GPU's outcome equal to the
model's on the tiny circuit; bad encodings are named by section and index; unusable arguments are
refused before any device work; the context proves as before after a check.  ptaus and keys are
module fixtures with fixed secrets.
"""
import json
import os
import random
import shutil
import subprocess
import sys
import types

import pytest

import keycheck_model as model
import keycheck_tampers as tp
import r1cs_systems as rs
from oracle import groth16 as og
from oracle import witness as ow
from test_ptau_cpu import tiny_circuit
from zkfl import circuits, groth16, native, ptau, zkey
from zkfl.field import R
from zkfl.r1cs_file import read_r1cs

pytestmark = pytest.mark.gpu

TAU, ALPHA, BETA, D1, D2 = 0x2468ACE13579, 0x1111, 0x2222, 0x3333, 0x4444
ALL_PASS = {c: "pass" for c in native.KEY_CHECKS}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(os.path.dirname(os.path.abspath(zkey.__file__)))


def _sc(vals) -> bytes:
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


class Case:
    """A system, its .r1cs bytes, fixed rho / sigma and the resident r1cs (made on first use)."""

    def __init__(self, ctx, cs, r1cs_bytes, seed):
        self.ctx, self.cs, self.r1cs = ctx, cs, r1cs_bytes
        self.n = zkey.domain_size_for(cs)
        rng = random.Random(seed)
        self.rho = [rng.randrange(R) for _ in range(cs.n_wires)]
        self.sigma = [rng.randrange(R) for _ in range(self.n)]
        self._dev = None

    @property
    def dev(self):
        if self._dev is None:
            self._dev = native.R1cs(self.ctx, self.r1cs)
        return self._dev

    def check(self, zk, pt, fixed=True):
        blocks = zkey.ptau_blocks(self.cs, pt)
        if fixed:
            return self.dev.check_key(zk, blocks, _sc(self.rho), _sc(self.sigma))
        return self.dev.check_key(zk, blocks)

    def both(self, zk, pt):
        """the report with fixed rho, sigma after asserting that drawn ones give the same verdicts"""
        rep = self.check(zk, pt)
        assert self.check(zk, pt, fixed=False).checks == rep.checks
        return rep


@pytest.fixture(scope="module")
def world():
    mp = pytest.MonkeyPatch()
    mp.setenv("ZKFL_DETERMINISTIC_SETUP", "1")
    ctx = native.Context(0)

    def pot(power, tau=TAU):
        return ptau.prepare_phase2(ptau.contribute(ptau.new(power), ctx, tau, ALPHA, BETA), ctx)
    w = types.SimpleNamespace(ctx=ctx, pot={p: pot(p) for p in (3, 4, 9, 10)},
                              pot_other={p: pot(p, TAU + 1) for p in (4, 10)})
    b = tiny_circuit()
    w.tiny = Case(ctx, b, b.r1cs_bytes(), 1)
    zk0 = zkey.setup_from_ptau(b, w.pot[4], ctx)
    zk1 = zkey.zkey_contribute(zk0, ctx, D1)
    w.tiny_keys = {0: zk0, 1: zk1, 2: zkey.zkey_contribute(zk1, ctx, D2)}
    n_wires, cons, _ = rs.product_system(257, random.Random(77))
    raw = rs.write_r1cs(n_wires, cons, n_pub_out=1, n_pub_in=1, n_prv_in=n_wires - 3)
    w.big = Case(ctx, read_r1cs(raw), raw, 2)
    assert (w.big.cs.n_wires, w.big.n) == (306, 512)
    w.big_key = zkey.zkey_contribute(zkey.setup_from_ptau(w.big.cs, w.pot[10], ctx), ctx, D1)
    yield w
    ctx.close()
    mp.undo()


# ---------------------------------------------------------------------------
# honest keys
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("contributions", [0, 1, 2])
def test_tiny_keys_pass(world, contributions):
    rep = world.tiny.both(world.tiny_keys[contributions], world.pot[4])
    assert rep.ok and rep.checks == ALL_PASS and rep.error == ""


def test_tiny_at_full_power_passes(world):
    """ptau power 3 == the circuit's: H0 comes from snarkjs's truncated top block."""
    zk = zkey.zkey_contribute(zkey.setup_from_ptau(world.tiny.cs, world.pot[3], world.ctx), world.ctx, D1)
    assert world.tiny.both(zk, world.pot[3]).checks == ALL_PASS


def test_dev_key_with_gamma_passes(world):
    """The known-tau dev ceremony with the ptau's tau, alpha, beta and gamma = 7, delta = 11."""
    zk = zkey.groth16_setup(world.tiny.cs, world.ctx, zkey.Toxic(tau=TAU, alpha=ALPHA, beta=BETA, gamma=7, delta=11))
    assert world.tiny.both(zk, world.pot[4]).checks == ALL_PASS


def test_poseidon_key_passes(world):
    """domain 2^8 over a power-9 ptau; about a third of B1 / B2 is infinity."""
    b = circuits.build("poseidon_hash2")
    case = Case(world.ctx, b, b.r1cs_bytes(), 3)
    zk = zkey.zkey_contribute(zkey.setup_from_ptau(b, world.pot[9], world.ctx), world.ctx, D1)
    assert case.n == 256 and len(tp.live(zk, 6)) < 0.8 * b.n_wires
    assert case.both(zk, world.pot[9]).checks == ALL_PASS
    case.dev.close()


@pytest.mark.parametrize("name", ["wire_twice", "empty_a", "empty_b", "multi_c", "no_terms", "rows_16"])
def test_edge_system_keys_pass(world, name):
    """Shapes the builder never writes, with one public output and one public input so the public
    rows exist: the key comes from read_r1cs's merged terms, the check reads the file's own."""
    n_wires, cons, _ = rs.edge_systems()[name]
    raw = rs.write_r1cs(n_wires, cons, n_pub_out=1, n_pub_in=1, n_prv_in=n_wires - 3)
    case = Case(world.ctx, read_r1cs(raw), raw, 4)
    zk = zkey.zkey_contribute(zkey.setup_from_ptau(case.cs, world.pot[10], world.ctx), world.ctx, D1)
    assert case.both(zk, world.pot[10]).checks == ALL_PASS
    case.dev.close()


def test_big_key_passes(world):
    assert world.big.both(world.big_key, world.pot[10]).checks == ALL_PASS


# ---------------------------------------------------------------------------
# tamper matrix
# ---------------------------------------------------------------------------
MATRIX = ["A_swapped", "B1_doubled", "B2_replaced", "IC_changed", "C_scaled", "H_swapped", "coef_plus_one",
          "term_moved", "delta1_scaled", "alpha1_replaced"]


def _assert_outcome(rep, want):
    assert rep.checks == want
    assert rep.rc == -8 and not rep.ok
    first = next(c for c in native.KEY_CHECKS if want[c] == "fail")
    assert rep.first_failed == first and f"zkey check: {first} fails" in rep.error


@pytest.mark.parametrize("name", MATRIX)
def test_tamper_tiny_equals_model(world, name):
    t = world.tiny
    zk = tp.TAMPERS[name][0](world.tiny_keys[1])
    rep = t.both(zk, world.pot[4])
    _assert_outcome(rep, tp.expected(name))
    m = model.check(t.cs.cons, t.cs.n_wires, t.cs.n_public, world.pot[4], zk, t.rho, t.sigma)
    assert rep.checks == m["checks"] and rep.coef == m["coef"] and rep.point == m["point"]


@pytest.mark.parametrize("name", MATRIX)
def test_tamper_big(world, name):
    _assert_outcome(world.big.both(tp.TAMPERS[name][0](world.big_key), world.pot[10]), tp.expected(name))


def _other_system(case, ctx, pt):
    """the key of the same system with one A coefficient of a private wire changed"""
    cons = [tuple(dict(m) for m in con) for con in case.cs.cons]
    j, w = next((j, w) for j, con in enumerate(cons) for w in con[0] if w > case.cs.n_public)
    cons[j][0][w] = (cons[j][0][w] + 1) % R
    other = types.SimpleNamespace(cons=cons, n_wires=case.cs.n_wires, n_public=case.cs.n_public,
                                  n_constraints=len(cons))
    return zkey.zkey_contribute(zkey.setup_from_ptau(other, pt, ctx), ctx, D1), cons


@pytest.mark.parametrize("which,power", [("tiny", 4), ("big", 10)])
def test_key_of_another_system(world, which, power):
    case = getattr(world, which)
    zk, _ = _other_system(case, world.ctx, world.pot[power])
    _assert_outcome(case.both(zk, world.pot[power]), dict(ALL_PASS, coefficients="fail", A="fail", C="fail"))


@pytest.mark.parametrize("which,power", [("tiny", 4), ("big", 10)])
def test_ptau_of_another_tau(world, which, power):
    """the same alpha and beta, another tau: the header holds, every query fails"""
    case = getattr(world, which)
    zk = world.tiny_keys[1] if which == "tiny" else world.big_key
    want = dict(ALL_PASS, A="fail", B1="fail", B2="fail", IC="fail", C="fail", H="fail")
    _assert_outcome(case.both(zk, world.pot_other[power]), want)


# ---------------------------------------------------------------------------
# points
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("section,index", [(5, 0), (5, 63), (5, 64), (5, 255), (5, 256), (5, 305),
                                           (9, 0), (9, 63), (9, 64), (9, 255), (9, 256), (9, 511)])
def test_off_curve_point_is_named(world, section, index):
    """Section 5 of this key is sparse (the product wires have no A term), section 9 is dense: its
    indices cross the kernel's wave and workgroup edges."""
    rep = world.big.check(tp.off_curve(world.big_key, section, index), world.pot[10])
    skipped = "A" if section == 5 else "H"
    _assert_outcome(rep, dict(ALL_PASS, points="fail", **{skipped: "not run"}))
    assert rep.point == (section, index, 1)
    assert f"section {section} point {index}" in rep.error


def test_two_bad_points_name_the_lowest(world):
    zk = tp.off_curve(tp.off_curve(world.big_key, 9, 300), 9, 70)
    rep = world.big.check(zk, world.pot[10])
    assert rep.point == (9, 70, 2) and rep.checks["H"] == "not run"


def test_coordinate_plus_q(world):
    i = tp.live(world.big_key, 5)[3]
    rep = world.big.check(tp.plus_q(world.big_key, 5, i), world.pot[10])
    _assert_outcome(rep, dict(ALL_PASS, points="fail", A="not run"))
    assert rep.point == (5, i, 1)


def test_twist_point_outside_g2(world):
    i = tp.live(world.big_key, 7)[5]
    rep = world.big.check(tp.put_point(world.big_key, 7, i, tp.twist_point_outside_g2()), world.pot[10])
    _assert_outcome(rep, dict(ALL_PASS, points="fail", B2="not run"))
    assert rep.point == (7, i, 1)


def test_infinity_delta2(world):
    rep = world.big.check(tp.hdr_raw(world.big_key, "delta2", bytes(128)), world.pot[10])
    _assert_outcome(rep, dict(ALL_PASS, header="fail", C="not run", H="not run"))
    assert "delta2 is infinity" in rep.error


def test_encoding_tampers_equal_model(world):
    t = world.tiny
    for name in ("A_off_curve", "A_plus_q", "B2_outside_g2", "delta2_infinity"):
        zk = tp.TAMPERS[name][0](world.tiny_keys[1])
        rep = t.check(zk, world.pot[4])
        m = model.check(t.cs.cons, t.cs.n_wires, t.cs.n_public, world.pot[4], zk, t.rho, t.sigma)
        assert rep.checks == m["checks"] == tp.expected(name), name
        assert rep.point == m["point"], name


# ---------------------------------------------------------------------------
# errors, before any device work
# ---------------------------------------------------------------------------
def _code(fn):
    with pytest.raises(native.ZkflError) as e:
        fn()
    return e.value.code


def test_errors(world):
    t, zk, pt = world.tiny, world.tiny_keys[1], world.pot[4]
    o = tp.zsecs(zk)[2][0] + 76
    assert _code(lambda: t.check(tp.patch(zk, o, (t.cs.n_public + 1).to_bytes(4, "little")), pt)) == -4
    blocks = zkey.ptau_blocks(t.cs, pt)
    assert _code(lambda: t.dev.check_key(zk, dict(blocks, La=blocks["La"][:-64]))) == -1
    assert _code(lambda: t.dev.check_key(zk, dict(blocks, power=4))) == -4
    rho = list(t.rho)
    rho[3] = R
    assert _code(lambda: t.dev.check_key(zk, blocks, _sc(rho), _sc(t.sigma))) == -1
    sigma = list(t.sigma)
    sigma[-1] = (1 << 256) - 1
    assert _code(lambda: t.dev.check_key(zk, blocks, _sc(t.rho), _sc(sigma))) == -1
    with native.Context(0) as other, native.R1cs(other, t.r1cs) as foreign:
        view = native.PtauView()
        rep = native.ZkeyReport()
        rc = native.lib().zkfl_zkey_check(world.ctx.h, foreign.h, zk, len(zk), view, None, None, rep)
        assert rc == -1 and b"another context" in native.lib().zkfl_last_error()
    with pytest.raises(ValueError, match="not prepared"):
        groth16.zkey_check(t.r1cs, ptau.new(4), zk, world.ctx)


# ---------------------------------------------------------------------------
# after a check
# ---------------------------------------------------------------------------
def test_context_still_proves_and_r1cs_is_shared(world):
    t, zk = world.tiny, world.tiny_keys[1]
    assert t.check(zk, world.pot[4]).ok
    w = ow.evaluate(t.cs, {"x": 3, "z": 7})
    wt = zkey.wtns_bytes(w)
    assert t.dev.check([wt])[0].ok                       # the same resident r1cs serves `wtns check`
    bad = list(w)
    bad[-1] = (bad[-1] + 1) % R
    assert not t.dev.check([zkey.wtns_bytes(bad)])[0].ok
    assert t.check(zk, world.pot[4]).ok                  # and the key check again after it
    r, s = 0xABCDEF, 0x123457
    key = native.ProvingKey(world.ctx, zk)
    proof, pub = key.prove(wt, r.to_bytes(32, "little") + s.to_bytes(32, "little"))
    key.close()
    assert proof == og.proof_bytes(og.prove(og.parse_zkey(zk), w, r=r, s=s)) and pub == [3 ** 3 + 21 + 5]


def test_profiler_stages(world):
    world.ctx.set_profiling(True)
    try:
        world.ctx.profile_reset()
        assert world.big.check(world.big_key, world.pot[10]).ok
        for stage in ("keycheck_points", "keycheck_rows", "keycheck_msm", "keycheck_pairing"):
            ms, launches, _, _ = world.ctx.profile(stage)
            assert launches == 1 and ms > 0, stage
    finally:
        world.ctx.profile_reset()
        world.ctx.set_profiling(False)


# ---------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------
def _run(argv, cwd):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT, ZKFL_PYTHON=sys.executable)
    return subprocess.run(argv, cwd=cwd, env=env, capture_output=True, text=True, timeout=300)


def test_cli_strings(world, tmp_path):
    """`python -m zkfl zkey check`, `prove --check-key` and, where node is present, the shim's
    `snarkjs zkey check`, each on a good and on a bad key."""
    t = world.tiny
    files = {"c.r1cs": t.r1cs, "pot.ptau": world.pot[4], "good.zkey": world.tiny_keys[1],
             "bad.zkey": tp.TAMPERS["C_scaled"][0](world.tiny_keys[1]),
             "w.wtns": zkey.wtns_bytes(ow.evaluate(t.cs, {"x": 3, "z": 7}))}
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
    py = [sys.executable, "-m", "zkfl"]
    good = _run(py + ["zkey", "check", "c.r1cs", "pot.ptau", "good.zkey"], tmp_path)
    assert good.returncode == 0, good.stderr
    assert [ln.split(":")[0] for ln in good.stdout.splitlines()[:9]] == list(native.KEY_CHECKS)
    bad = _run(py + ["zkey", "check", "c.r1cs", "pot.ptau", "bad.zkey"], tmp_path)
    assert bad.returncode == 1 and "C: fail" in bad.stdout and "zkey check: C fails" in bad.stderr
    ok = _run(py + ["prove", "good.zkey", "w.wtns", "proof.json", "public.json", "--check-key", "c.r1cs", "pot.ptau"],
              tmp_path)
    assert ok.returncode == 0, ok.stderr
    assert json.load(open(tmp_path / "public.json")) == [str(3 ** 3 + 21 + 5)]
    no = _run(py + ["prove", "bad.zkey", "w.wtns", "proof2.json", "public2.json", "--check-key", "c.r1cs", "pot.ptau"],
              tmp_path)
    assert no.returncode == 1 and "ZKFL_E_KEY" in no.stderr and not (tmp_path / "proof2.json").exists()
    node = shutil.which("node")
    shim = os.path.join(PKG, "node", "snarkjs_shim.js")
    if node and os.path.exists(os.path.join(PKG, "node", "zkfl.node")):
        assert _run([node, shim, "zkey", "check", "c.r1cs", "pot.ptau", "good.zkey"], tmp_path).returncode == 0
        assert _run([node, shim, "zkey", "check", "c.r1cs", "pot.ptau", "bad.zkey"], tmp_path).returncode == 1
