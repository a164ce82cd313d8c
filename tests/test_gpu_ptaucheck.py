"""`powersoftau check` on the GPU (zkfl_ptau_check, csrc/ptaucheck.hip) -- MI355X.

Is a .ptau a well-formed Powers of Tau for some tau, alpha and beta, with sections 12-15 the Lagrange
form of sections 2-5?  `groth16 setup` and `zkey check` read sections 12-15 of whatever ptau they are
given (tests/full_system_simulation.mjs:677-695).  Files come from zkfl.ptau.new / contribute /
prepare_phase2 with fixed secrets.  Honest files of 0, 1 and 2 contributions pass; the tamper table of
tests/ptaucheck_tampers.py fails exactly its checks (the contract tests/test_ptaucheck_cpu.py holds
the CPU model to) with the GPU's outcome equal to the model's under the same rnd, in one chunk and in
chunks of 8 points; power 1 and power 9 cover the smallest file and scalar kernels of several
workgroups; unusable arguments are refused before any device work; the context proves as before
after a check; `zkey check --check-ptau` closes the hole a plain `zkey check` leaves.
"""
import os
import random
import shutil
import subprocess
import sys
import types

import pytest

import ptaucheck_model as model
import ptaucheck_tampers as tp
from oracle import groth16 as og
from oracle import witness as ow
from test_ptau_cpu import tiny_circuit
from test_ptaucheck_cpu import make_rnd
from zkfl import groth16, native, ptau, zkey
from zkfl.field import R

pytestmark = pytest.mark.gpu

SECRETS = [(0x2468ACE13579, 0x1111, 0x2222), (0xFEDCBA987, 0x3333, 0x4444)]
ALL_PASS = {c: "pass" for c in native.PTAU_CHECKS}
UNPREPARED = {c: "not run" if c in native.PTAU_LAGRANGE_CHECKS else "pass" for c in native.PTAU_CHECKS}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(os.path.dirname(os.path.abspath(zkey.__file__)))
TABLE = tp.table(4)
CHUNKS = {"one_chunk": 0, "chunks_of_8": 8}


def sections_chunks(power, prepared, chunk):
    """chunk passes of a file: every section of 2-6, 12-15 in ceil(count / chunk) passes"""
    n = 1 << power
    counts = [2 * n - 1, n, n, n, 1] + ([4 * n - 1, 2 * n - 1, 2 * n - 1, 2 * n - 1] if prepared else [])
    return sum(-(-c // chunk) for c in counts)


@pytest.fixture(scope="module")
def world():
    mp = pytest.MonkeyPatch()
    mp.setenv("ZKFL_DETERMINISTIC_SETUP", "1")
    ctx = native.Context(0)

    def pot(power, k, secrets=SECRETS):
        buf = ptau.new(power)
        for tau, alpha, beta in secrets[:k]:
            buf = ptau.contribute(buf, ctx, tau, alpha, beta)
        return ptau.prepare_phase2(buf, ctx)
    w = types.SimpleNamespace(ctx=ctx, pot={(p, k): pot(p, k) for p, k in ((1, 1), (4, 0), (4, 1), (4, 2), (9, 2))})
    w.env = types.SimpleNamespace(prepare=lambda buf: ptau.prepare_phase2(buf, ctx),
                                  other=pot(4, 1, [(0x99887766, 0x1111, 0x2222)]))
    w.rnd = {p: make_rnd(p, 1000 + p) for p in (1, 4, 9)}
    w.model = {}

    def expect(name, buf):
        """the model's outcome for this file under rnd[4], computed once"""
        if name not in w.model:
            w.model[name] = model.check(buf, w.rnd[4])
        return w.model[name]
    w.expect = expect
    yield w
    ctx.close()
    mp.undo()


def _assert_fails(rep, want):
    assert rep.checks == want
    assert rep.rc == -8 and not rep.ok
    first = next(c for c in native.PTAU_CHECKS if want[c] == "fail")
    assert rep.first_failed == first and f"powersoftau check: {first} fails" in rep.error


# ---------------------------------------------------------------------------
# honest files
# ---------------------------------------------------------------------------
def test_power_1(world):
    """Three points in section 2, blocks of 1, 2 and 4 in section 12."""
    buf = world.pot[(1, 1)]
    rep = world.ctx.check_ptau(buf, world.rnd[1])
    assert rep.ok and rep.checks == ALL_PASS and rep.prepared and rep.power == 1 and rep.error == ""
    assert rep.checks == model.check(buf, world.rnd[1])["checks"]
    assert world.ctx.check_ptau(buf).ok
    for chunk in (1, 2, 3):
        assert world.ctx.check_ptau(buf, world.rnd[1], chunk).checks == ALL_PASS
    bad = tp.replaced(buf, 12, 5)
    want = dict(ALL_PASS, L_TAU_G1="fail")
    _assert_fails(world.ctx.check_ptau(bad, world.rnd[1]), want)
    assert model.check(bad, world.rnd[1])["checks"] == want
    _assert_fails(world.ctx.check_ptau(tp.replaced(buf, 2, 2), world.rnd[1], 2), dict(ALL_PASS, TAU_G1="fail", L_TAU_G1="fail"))


@pytest.mark.parametrize("how", sorted(CHUNKS))
@pytest.mark.parametrize("contributions", [0, 1, 2])
def test_honest_files_pass(world, contributions, how):
    """`powersoftau new` (tau = 1: all but one point of every Lagrange block is infinity, so most
    compacted chunks are empty), one and two contributions."""
    buf = world.pot[(4, contributions)]
    rep = world.ctx.check_ptau(buf, world.rnd[4], CHUNKS[how])
    assert rep.ok and rep.checks == ALL_PASS and rep.prepared and rep.power == 4
    assert rep.checks == world.expect(f"honest{contributions}", buf)["checks"]
    assert rep.chunks == sections_chunks(4, True, CHUNKS[how] or 1 << 20)


def test_chunks_are_counted(world):
    """Section 2 of a power-4 file splits 8 + 8 + 8 + 7 and section 12 is 63 points."""
    buf = world.pot[(4, 2)]
    one = world.ctx.check_ptau(buf, world.rnd[4]).chunks
    many = world.ctx.check_ptau(buf, world.rnd[4], 8).chunks
    assert one == 9 and many == 4 + 2 + 2 + 2 + 1 + 8 + 4 + 4 + 4 and many > one


@pytest.mark.parametrize("how", sorted(CHUNKS))
@pytest.mark.parametrize("name", sorted(tp.PASSES))
def test_valid_variants_pass(world, name, how):
    buf = tp.PASSES[name](world.pot[(4, 2)], world.env)
    rep = world.ctx.check_ptau(buf, world.rnd[4], CHUNKS[how])
    want = UNPREPARED if name == "unprepared" else ALL_PASS
    assert rep.ok and rep.rc == 0 and rep.checks == want and rep.prepared == (name != "unprepared")
    assert rep.checks == world.expect("variant_" + name, buf)["checks"]
    if name == "unprepared":
        assert rep.chunks == sections_chunks(4, False, CHUNKS[how] or 1 << 20)
        assert [ln for ln in rep.lines() if ln.startswith("L_")] == [f"{c}: not run (not prepared)"
                                                                    for c in native.PTAU_LAGRANGE_CHECKS]


def test_drawn_scalars(world):
    """rnd = NULL: the library draws z, gamma and rho itself"""
    buf = world.pot[(4, 2)]
    for chunk in (0, 8):
        assert world.ctx.check_ptau(buf, None, chunk).checks == ALL_PASS
        _assert_fails(world.ctx.check_ptau(tp.replaced(buf, 14, 9), None, chunk), dict(ALL_PASS, L_ALPHA_G1="fail"))
        _assert_fails(world.ctx.check_ptau(tp.replaced(buf, 3, 9), None, chunk),
                      dict(ALL_PASS, TAU_G2="fail", L_TAU_G2="fail"))


# ---------------------------------------------------------------------------
# tamper table: the GPU equals the model, in one chunk and in chunks of 8
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("how", sorted(CHUNKS))
@pytest.mark.parametrize("name", sorted(TABLE))
def test_tamper_equals_model(world, name, how):
    edit, _, _, point = TABLE[name]
    buf = edit(world.pot[(4, 2)], world.env)
    rep = world.ctx.check_ptau(buf, world.rnd[4], CHUNKS[how])
    want = tp.expected(TABLE, name)
    _assert_fails(rep, want)
    m = world.expect(name, buf)
    assert rep.checks == m["checks"] and rep.point == m["point"] == point
    assert rep.status == m["status"]
    if point:
        assert f"section {point[0]} point {point[1]}" in rep.error


@pytest.mark.parametrize("section,index", [(2, 7), (2, 8), (2, 30), (12, 0), (12, 2), (12, 14), (12, 15), (12, 62)])
def test_tamper_at_chunk_edges(world, section, index):
    """Chunks of 8: section 2's indices 7 | 8 sit on either side of a chunk edge (the chain's
    overlapping scalar) and 30 is the last point; section 12's positions 2 and 14 end a level, 15
    starts the next chunk and level, 62 is the last position."""
    buf = tp.replaced(world.pot[(4, 2)], section, index)
    want = dict(ALL_PASS, L_TAU_G1="fail") if section == 12 else dict(ALL_PASS, TAU_G1="fail", L_TAU_G1="fail")
    for chunk in (8, 0):
        _assert_fails(world.ctx.check_ptau(buf, world.rnd[4], chunk), want)
    assert world.expect(f"edge_{section}_{index}", buf)["checks"] == want
    bad = tp.off_curve(world.pot[(4, 2)], section, index)
    rep = world.ctx.check_ptau(bad, world.rnd[4], 8)
    assert rep.point == (section, index, 1)
    assert rep.checks == dict(ALL_PASS, POINTS="fail", **{c: "not run" for c in tp.GATED[section]})


def test_two_bad_points_in_two_chunks_name_the_lowest(world):
    buf = tp.off_curve(tp.off_curve(world.pot[(4, 2)], 12, 50), 12, 13)
    for chunk in (8, 0):
        rep = world.ctx.check_ptau(buf, world.rnd[4], chunk)
        assert rep.point == (12, 13, 2) and rep.checks["L_TAU_G1"] == "not run"


# ---------------------------------------------------------------------------
# power 9: scalar kernels of several workgroups, lane runs across level boundaries
# ---------------------------------------------------------------------------
def test_power_9(world):
    buf = world.pot[(9, 2)]
    for chunk in (0, 300):
        rep = world.ctx.check_ptau(buf, world.rnd[9], chunk)
        assert rep.ok and rep.checks == ALL_PASS and rep.power == 9
        assert rep.chunks == sections_chunks(9, True, chunk or 1 << 20)
    assert world.ctx.check_ptau(buf).ok


@pytest.mark.parametrize("section,index,fails", [
    (12, 1022, {"L_TAU_G1"}),                 # the last position of level 9, mid-run of its lane
    (12, 2046, {"L_TAU_G1"}),                 # the last position of the section
    (13, 700, {"L_TAU_G2"}),
    (2, 777, {"TAU_G1", "L_TAU_G1"}),
    (5, 511, {"BETA_G1", "L_BETA_G1"})])
def test_power_9_tampers(world, section, index, fails):
    buf = tp.replaced(world.pot[(9, 2)], section, index)
    want = {c: "fail" if c in fails else "pass" for c in native.PTAU_CHECKS}
    _assert_fails(world.ctx.check_ptau(buf, world.rnd[9]), want)
    _assert_fails(world.ctx.check_ptau(buf, world.rnd[9], 300), want)


def test_power_9_off_curve(world):
    rep = world.ctx.check_ptau(tp.off_curve(world.pot[(9, 2)], 13, 333), world.rnd[9], 256)
    assert rep.point == (13, 333, 1) and rep.checks["L_TAU_G2"] == "not run" and rep.checks["TAU_G2"] == "pass"


# ---------------------------------------------------------------------------
# errors, before any device work
# ---------------------------------------------------------------------------
def _code(fn):
    with pytest.raises(native.ZkflError) as e:
        fn()
    return e.value.code


def _with(rnd, i, value):
    return rnd[:32 * i] + int(value).to_bytes(32, "little") + rnd[32 * (i + 1):]


def test_errors(world):
    buf, rnd = world.pot[(4, 1)], world.rnd[4]
    ck = world.ctx.check_ptau
    assert _code(lambda: ck(buf, _with(rnd, 0, R))) == -1                          # z >= r
    assert _code(lambda: ck(buf, _with(rnd, 3, R))) == -1                          # a gamma >= r
    assert _code(lambda: ck(buf, _with(rnd, len(rnd) // 32 - 1, (1 << 256) - 1))) == -1   # the last rho
    assert "not < r" in str(pytest.raises(native.ZkflError, lambda: ck(buf, _with(rnd, 9, R))).value)
    from oracle import bn254 as bn
    for z in (0, 1, R - 1, bn.FR_W[5], pow(bn.FR_W[5], 7, R), bn.FR_W[3]):          # on the 2n = 32 domain
        assert _code(lambda z=z: ck(buf, _with(rnd, 0, z))) == -1
    assert ck(buf, _with(rnd, 0, bn.FR_W[6])).ok                                    # order 64: off it
    L = native.lib()
    rep = native.PtauReportC()
    assert L.zkfl_ptau_check(None, buf, len(buf), None, 0, rep) == -1
    assert L.zkfl_ptau_check(world.ctx.h, None, 0, None, 0, rep) == -1
    assert L.zkfl_ptau_check(world.ctx.h, buf, len(buf), None, 0, None) == 0        # a null report is allowed
    assert _code(lambda: ck(buf[:200])) == -2
    assert _code(lambda: ck(b"zkey" + buf[4:])) == -2
    secs = tp.split(buf)
    assert _code(lambda: ck(tp.binfile({t: s for t, s in secs.items() if t != 13}))) == -2
    assert _code(lambda: ck(tp.binfile({**secs, 4: secs[4][:-64]}))) == -4


def test_buffers_and_mapped_files(world, tmp_path):
    """bytes, a bytearray and a mapped file give the same report; a path is mapped, not read"""
    buf = world.pot[(4, 2)]
    path = tmp_path / "pot.ptau"
    path.write_bytes(buf)
    want = world.ctx.check_ptau(buf, world.rnd[4]).status
    assert world.ctx.check_ptau(bytearray(buf), world.rnd[4]).status == want
    assert world.ctx.check_ptau(memoryview(buf), world.rnd[4]).status == want
    rep = groth16.ptau_check(str(path), world.ctx)
    assert rep.ok and rep.checks == ALL_PASS
    assert native.ptau_header(bytearray(buf)) == dict(power=4, ceremony_power=4, prepared=1, contributions=2)
    (tmp_path / "bad.ptau").write_bytes(tp.replaced(buf, 15, 20))
    assert groth16.ptau_check(tmp_path / "bad.ptau", world.ctx).failed == ["L_BETA_G1"]
    assert "ptau_check" in groth16.__all__


# ---------------------------------------------------------------------------
# after a check
# ---------------------------------------------------------------------------
def test_context_still_proves(world):
    assert world.ctx.check_ptau(world.pot[(4, 2)]).ok
    b = tiny_circuit()
    zk = zkey.zkey_contribute(zkey.setup_from_ptau(b, world.pot[(4, 2)], world.ctx), world.ctx, 0x5555)
    w = ow.evaluate(b, {"x": 3, "z": 7})
    r, s = 0xABCDEF, 0x123457
    key = native.ProvingKey(world.ctx, zk)
    proof, pub = key.prove(zkey.wtns_bytes(w), r.to_bytes(32, "little") + s.to_bytes(32, "little"))
    key.close()
    assert proof == og.proof_bytes(og.prove(og.parse_zkey(zk), w, r=r, s=s)) and pub == [3 ** 3 + 21 + 5]
    assert world.ctx.check_ptau(world.pot[(4, 2)], world.rnd[4], 8).ok


def test_profiler_stages(world):
    world.ctx.set_profiling(True)
    try:
        world.ctx.profile_reset()
        rep = world.ctx.check_ptau(world.pot[(4, 2)], world.rnd[4], 8)
        assert rep.ok
        ms, launches, units, _ = world.ctx.profile("ptaucheck_points")
        assert launches == rep.chunks and ms > 0 and units == 31 + 3 * 16 + 1 + 63 + 3 * 31
        for stage in ("ptaucheck_scalars", "ptaucheck_msm"):
            ms, launches, _, _ = world.ctx.profile(stage)
            assert launches == rep.chunks - 1 and ms > 0, stage      # section 6 has no MSM
        ms, launches, _, _ = world.ctx.profile("ptaucheck_pairing")
        assert launches == 1 and ms > 0
    finally:
        world.ctx.profile_reset()
        world.ctx.set_profiling(False)


# ---------------------------------------------------------------------------
# the hole being closed: a key over a ptau with a bad Lagrange point
# ---------------------------------------------------------------------------
def test_zkey_check_with_check_ptau(world):
    """A ptau whose section 12 has one altered point in the block `groth16 setup` reads: the key set
    up from it passes a plain `zkey check` (both sides of its equations read the same block) and is
    stopped by `check_ptau=True`, with the ptau check's report."""
    b = tiny_circuit()
    n = zkey.domain_size_for(b)
    bad_pot = tp.replaced(world.pot[(4, 2)], 12, n - 1 + 2)          # block log2(n) of section 12, point 2
    zk = zkey.zkey_contribute(zkey.setup_from_ptau(b, bad_pot, world.ctx), world.ctx, 0x5555)
    r1 = b.r1cs_bytes()
    plain = groth16.zkey_check(r1, bad_pot, zk, world.ctx)
    assert plain.ok and isinstance(plain, native.KeyReport)
    rep = groth16.zkey_check(r1, bad_pot, zk, world.ctx, check_ptau=True)
    assert not rep.ok and isinstance(rep, native.PtauReport) and rep.failed == ["L_TAU_G1"]
    assert "powersoftau check: L_TAU_G1 fails" in rep.error
    good = groth16.zkey_check(r1, world.pot[(4, 2)], zk, world.ctx, check_ptau=True)
    assert isinstance(good, native.KeyReport) and not good.ok     # the sound ptau: now the key is what fails
    zk_good = zkey.zkey_contribute(zkey.setup_from_ptau(b, world.pot[(4, 2)], world.ctx), world.ctx, 0x5555)
    assert groth16.zkey_check(r1, world.pot[(4, 2)], zk_good, world.ctx, check_ptau=True).ok


# ---------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------
def _run(argv, cwd):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT, ZKFL_PYTHON=sys.executable)
    return subprocess.run(argv, cwd=cwd, env=env, capture_output=True, text=True, timeout=300)


def test_cli_strings(world, tmp_path):
    """`python -m zkfl powersoftau check` on a good, an unprepared, a bad and a malformed file (exit 0,
    0, 1, 2), `zkey check --check-ptau`, and, where node is present, the shim's string."""
    b = tiny_circuit()
    good = world.pot[(4, 2)]
    bad = tp.replaced(good, 12, zkey.domain_size_for(b) - 1 + 2)
    files = {"good.ptau": good, "raw.ptau": tp.unprepared(good), "bad.ptau": bad, "short.ptau": good[:300],
             "c.r1cs": b.r1cs_bytes(),
             "c.zkey": zkey.zkey_contribute(zkey.setup_from_ptau(b, bad, world.ctx), world.ctx, 0x5555)}
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
    py = [sys.executable, "-m", "zkfl"]
    out = _run(py + ["powersoftau", "check", "good.ptau"], tmp_path)
    assert out.returncode == 0, out.stderr
    assert out.stdout.splitlines()[:11] == [f"{c}: pass" for c in native.PTAU_CHECKS]
    assert "PTAU IS A WELL-FORMED POWERS OF TAU" in out.stdout
    out = _run(py + ["powersoftau", "check", "raw.ptau"], tmp_path)
    assert out.returncode == 0, out.stderr
    assert out.stdout.splitlines()[7:11] == [f"{c}: not run (not prepared)" for c in native.PTAU_LAGRANGE_CHECKS]
    out = _run(py + ["powersoftau", "check", "bad.ptau"], tmp_path)
    assert out.returncode == 1 and "L_TAU_G1: fail" in out.stdout and "powersoftau check: L_TAU_G1 fails" in out.stderr
    out = _run(py + ["powersoftau", "check", "short.ptau"], tmp_path)
    assert out.returncode == 2 and "ZKFL_E_FORMAT" in out.stderr
    assert _run(py + ["powersoftau", "check"], tmp_path).returncode == 2
    plain = _run(py + ["zkey", "check", "c.r1cs", "bad.ptau", "c.zkey"], tmp_path)
    assert plain.returncode == 0, plain.stderr
    strict = _run(py + ["zkey", "check", "c.r1cs", "bad.ptau", "c.zkey", "--check-ptau"], tmp_path)
    assert strict.returncode == 1 and "L_TAU_G1: fail" in strict.stdout and "L_TAU_G1 fails" in strict.stderr


def test_shim_strings(world, tmp_path):
    """`npx snarkjs powersoftau check` through the shim and its in-process powersOfTau.check"""
    node = shutil.which("node")
    shim = os.path.join(PKG, "node", "snarkjs_shim.js")
    if not (node and os.path.exists(os.path.join(PKG, "node", "zkfl.node"))):
        pytest.skip("node or addon not available")
    good = world.pot[(4, 2)]
    (tmp_path / "good.ptau").write_bytes(good)
    (tmp_path / "bad.ptau").write_bytes(tp.replaced(good, 12, 9))
    assert _run([node, shim, "powersoftau", "check", "good.ptau"], tmp_path).returncode == 0
    assert _run([node, shim, "powersoftau", "check", "bad.ptau"], tmp_path).returncode == 1
    js = ("const s=require(process.argv[1]);"
          "s.powersOfTau.check('good.ptau').then((a)=>s.powersOfTau.check('bad.ptau').then((b)=>{"
          "console.log(a+' '+b);process.exit(0);}));")
    out = _run([node, "-e", js, shim], tmp_path)
    assert out.returncode == 0 and out.stdout.strip() == "true false", out.stderr
