"""`wtns check` on the GPU (zkfl_r1cs_load / zkfl_r1cs_check[_resident]) -- MI355X (-m gpu).

Every expected value is computed here with Python integers from the same constraints (the
builder's, or the hand-written systems of tests/r1cs_systems.py): the number of failing
constraints, the lowest failing index and the a, b, c values there must be equal, not close.
"""
import json
import os
import random
import shutil
import subprocess
import sys

import pytest

import r1cs_systems as rs
from oracle import witness as ow
from zkfl.field import R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "verifiable-federated-training-with-zero-knowledge-proofs-zk-fl-_amd")
E_ARG, E_MISMATCH, E_CONSTRAINT = -1, -4, -7


def _assert_report(rep, cons, w, what=""):
    n_failed, first, a, b, c = rs.expected(cons, w)
    assert rep.n_failed == n_failed, what
    assert rep.ok == (n_failed == 0), what
    if n_failed:
        assert (rep.first, rep.a, rep.b, rep.c) == (first, a, b, c), what


@pytest.fixture(scope="module")
def poseidon(gpu_ctx):
    """(builder, constraints as term lists, the oracle witness of {left: 1, right: 2}, loaded R1cs)"""
    from zkfl import circuits, native
    b = circuits.build("poseidon_hash2")
    cs = native.R1cs(gpu_ctx, b.r1cs_bytes())
    yield b, rs.lists_of(b.cons), ow.evaluate(b, {"left": 1, "right": 2}), cs
    cs.close()


def _bump(w, k):
    v = list(w)
    v[k] = (v[k] + 1) % R
    return v


def test_poseidon_hash2(poseidon):
    b, cons, w, cs = poseidon
    info = cs.info()
    assert (info["n_constraints"], info["n_terms"], info["n_wires"]) == (241, 6725, b.n_wires)
    assert max(len(lc) for con in cons for lc in con) == 61             # a row spans up to five 16-term chunks
    assert [j for j, con in enumerate(cons) if not con[2]] == [240]     # the only empty C row
    good = cs.check([rs.wtns_of(w)])[0]
    assert good.ok and good.n_failed == 0
    seen = {}
    for k in (1, 2, 3, 122, 243):
        v = _bump(w, k)
        rep = cs.check([rs.wtns_of(v)])[0]
        _assert_report(rep, cons, v, k)
        seen[k] = (rep.first, rep.n_failed)
    assert seen == {1: (240, 1), 2: (0, 2), 3: (3, 2), 122: (118, 2), 243: (239, 2)}


def _check_system(ctx, n_wires, cons, w, perturb):
    """The satisfying witness passes; each witness of `perturb` gets the report Python computes."""
    from zkfl import native
    with native.R1cs(ctx, rs.write_r1cs(n_wires, cons)) as cs:
        assert cs.info()["n_terms"] == rs.n_terms(cons)
        ws = [w] + perturb
        reps = cs.check([rs.wtns_of(v) for v in ws])
        assert reps[0].ok, "satisfying witness"
        for i, (rep, v) in enumerate(zip(reps, ws)):
            _assert_report(rep, cons, v, i)
        return reps


def test_hand_written_edge_systems(gpu_ctx):
    systems = rs.edge_systems()
    rng = random.Random(7)
    for name, (n_wires, cons, w) in systems.items():
        # every wire but the constant moved in turn (small systems), or a few random ones
        # (and the last wire, a C wire of its own in the generated systems)
        ks = range(1, n_wires) if n_wires <= 8 else [rng.randrange(1, n_wires) for _ in range(6)] + [n_wires - 1]
        reps = _check_system(gpu_ctx, n_wires, cons, w, [_bump(w, k) for k in ks])
        if name == "no_terms":
            assert all(r.ok for r in reps)      # every witness satisfies a system without terms
        else:
            assert any(not r.ok for r in reps[1:]), name
    starts = rs.row_starts(systems["rows_16"][1])
    assert all(starts[n] == {0, 1} for n in rs.ROW_LENGTHS)     # every length on and off a chunk start
    # r - 1 times r - 1: the largest product the field arithmetic meets
    n_wires, cons, w = systems["r_minus_1"]
    assert rs.evaluate(cons, w)[0] == (1, 1, 1)
    # an all-empty C column really has a == 0 or b == 0 per constraint; moving wire 1 breaks both
    n_wires, cons, w = systems["all_c_empty"]
    rep = _check_system(gpu_ctx, n_wires, cons, w, [_bump(w, 1)])[1]
    assert (rep.n_failed, rep.first, rep.c) == (2, 0, 0)


@pytest.mark.parametrize("m", [1, 63, 64, 65, 257])
def test_failure_positions(gpu_ctx, m):
    """A single failure at constraint 0, at m - 1, at 64 (wave edge) and 256 (workgroup edge), and
    every constraint failing: C_j is a wire of its own, so moving it breaks constraint j alone."""
    n_wires, cons, w = rs.product_system(m, random.Random(100 + m), max_terms=5)
    first_c = n_wires - m
    bad = []
    for j in sorted({0, m - 1, 64, 256}):
        if j < m:
            bad.append(_bump(w, first_c + j))
    everything = list(w)
    for j in range(m):
        everything[first_c + j] = (everything[first_c + j] + 1 + j) % R
    reps = _check_system(gpu_ctx, n_wires, cons, w, bad + [everything])
    singles = [(r.n_failed, r.first) for r in reps[1:-1]]
    assert singles == [(1, j) for j in sorted({0, m - 1, 64, 256}) if j < m]
    assert (reps[-1].n_failed, reps[-1].first) == (m, 0)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_systems(gpu_ctx, seed):
    """Random A and B rows of 0 to 40 terms, C_j one fresh wire = a_j b_j; then perturbed."""
    rng = random.Random(seed)
    m = rng.choice((90, 300, 700))
    n_wires, cons, w = rs.product_system(m, rng)
    perturb = [_bump(w, rng.randrange(1, n_wires)) for _ in range(5)]
    several = list(w)
    for _ in range(10):
        several[rng.randrange(1, n_wires)] = rng.randrange(R)
    reps = _check_system(gpu_ctx, n_wires, cons, w, perturb + [several])
    assert any(not r.ok for r in reps[1:])


def test_wide_terms(gpu_ctx):
    """More distinct coefficients than the spare bits of a term word can index: 2^16 + m + 1 wires
    leave 15 bits, i.e. 32,768 dictionary entries, and the ~37,000 terms here each carry a
    coefficient of their own -- the loader keeps one coefficient per term (wide terms)."""
    rng = random.Random(16)
    m = 900
    n_wires, cons, w = rs.product_system(m, rng, rows_a=[20] * m, rows_b=[20] * m, n_free=1 << 16, distinct=True)
    assert len({c for con in cons for lc in con for _, c in lc}) > 1 << 15 and (1 << 16) < n_wires <= 1 << 17
    perturb = [_bump(w, cons[j][0][0][0] or 1) for j in (0, 450, 899)] + [_bump(w, n_wires - 1)]
    reps = _check_system(gpu_ctx, n_wires, cons, w, perturb)
    assert (reps[-1].n_failed, reps[-1].first) == (1, m - 1) and not reps[1].ok


@pytest.fixture(scope="module")
def sgd(gpu_ctx):
    """sgd_verified(8,4,3): builder, constraints, the GPU witness engine's .wtns, loaded R1cs"""
    from zkfl import circuits, clients, native, wprog
    b = circuits.build("sgd_verified", 8, 4, 3, 1000)
    inp, _ = clients.Client(1, 8, 4, 3, clients.JsLcg(12345)).training_input(8, 1000, 100000000)
    wp = native.WitnessProgram(gpu_ctx, wprog.compile_program(b))
    wt = wp.compute([wprog.input_bytes(b, inp)])[0]
    wp.close()
    cs = native.R1cs(gpu_ctx, b.r1cs_bytes())
    yield b, rs.lists_of(b.cons), wt, cs
    cs.close()


def test_sgd_verified(sgd):
    from zkfl import zkey
    b, cons, wt, cs = sgd
    info = cs.info()
    assert (info["n_constraints"], info["n_terms"]) == (9903, 267849)
    assert sum(1 for con in cons if not con[2]) == 381
    assert cs.check([wt])[0].ok
    w = zkey.read_wtns(wt)
    k = 1 + b.n_pub_out + b.n_pub_in + 2      # a private input wire
    v = _bump(w, k)
    rep = cs.check([rs.wtns_of(v)])[0]
    assert not rep.ok
    _assert_report(rep, cons, v)


def test_batch(poseidon):
    from zkfl import native
    b, cons, w, cs = poseidon
    ws = [w, _bump(w, 3), w, _bump(w, 122), _bump(w, 1)]
    images = [rs.wtns_of(v) for v in ws]
    reps = cs.check(images)
    for i, (rep, v) in enumerate(zip(reps, ws)):
        _assert_report(rep, cons, v, i)
    assert [r.ok for r in reps] == [True, False, True, False, False]
    assert "witness 1:" in cs.last_error and "#3 " in cs.last_error
    # the return code, with reports and without
    L = native.lib()
    import ctypes as C
    arr = (C.c_char_p * 5)(*images)
    lens = (C.c_size_t * 5)(*[len(x) for x in images])
    out = (native.R1csReport * 5)()
    assert L.zkfl_r1cs_check(cs.ctx.h, cs.h, 5, arr, lens, out) == E_CONSTRAINT
    assert [r.n_failed for r in out] == [r.n_failed for r in reps]
    assert L.zkfl_r1cs_check(cs.ctx.h, cs.h, 5, arr, lens, None) == E_CONSTRAINT
    assert b"witness 1:" in L.zkfl_last_error()
    assert cs.check(images, reports=False) is False
    assert L.zkfl_r1cs_check(cs.ctx.h, cs.h, 2, (C.c_char_p * 2)(images[0], images[2]), lens, None) == 0
    assert cs.check([images[0], images[2]], reports=False) is True


def test_resident(gpu_ctx, poseidon):
    from zkfl import native, wprog, zkey
    b, cons, w, cs = poseidon
    zk = zkey.groth16_setup(b, gpu_ctx, zkey.Toxic(tau=31, alpha=3, beta=5, gamma=7, delta=11))
    key = native.ProvingKey(gpu_ctx, zk)
    wp = native.WitnessProgram(gpu_ctx, wprog.compile_program(b))
    res = wp.compute_resident(key, [wprog.input_bytes(b, {"left": 1, "right": 2})])
    assert cs.check_resident(res)[0].ok
    v = _bump(w, 122)
    up = key.upload(rs.wtns_of(v))
    got = cs.check_resident([res[0], up])
    assert "witness 1:" in cs.last_error
    ref = cs.check([rs.wtns_of(v)])[0]
    assert got[0].ok and not got[1].ok
    assert (got[1].n_failed, got[1].first, got[1].a, got[1].b, got[1].c) == (ref.n_failed, ref.first, ref.a, ref.b, ref.c)
    _assert_report(got[1], cons, v)
    for x in res + [up]:
        x.close()
    wp.close()
    key.close()


def test_errors(poseidon):
    from zkfl import native
    b, cons, w, cs = poseidon
    with pytest.raises(native.ZkflError) as e:
        cs.check([rs.wtns_of(w), rs.wtns_of(w + [5])])
    assert e.value.code == E_MISMATCH
    with pytest.raises(native.ZkflError) as e:
        cs.check([rs.wtns_of(w[:-1])])
    assert e.value.code == E_MISMATCH
    over = rs.wtns_of(w)
    at = len(over) - 32 * (len(w) - 7)      # wire 7's value
    over = over[:at] + R.to_bytes(32, "little") + over[at + 32:]
    with pytest.raises(native.ZkflError) as e:
        cs.check([over])
    assert e.value.code == E_ARG
    for w0 in (0, 2, R - 1):
        rep = cs.check([rs.wtns_of([w0] + w[1:])])[0]
        assert not rep.ok and rep.first == 0xFFFFFFFF == native.NO_CONSTRAINT
        assert "wire 0 is not 1" in cs.last_error
        assert cs.check([rs.wtns_of([w0] + w[1:])], reports=False) is False
    # a system without constants passes any scaled witness unless wire 0 is checked
    with native.R1cs(cs.ctx, rs.write_r1cs(3, [([], [], [])] * 2)) as empty:
        assert empty.check([rs.wtns_of([1, 5, 6])])[0].ok
        assert empty.check([rs.wtns_of([0, 5, 6])])[0].first == 0xFFFFFFFF


def _run(cmd, cwd, ok=True):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run(cmd, cwd=cwd, shell=True, capture_output=True, text=True, timeout=180, env=env)
    if ok:
        assert p.returncode == 0, f"{cmd}\n{p.stdout}\n{p.stderr}"
    return p


@pytest.fixture(scope="module")
def files(tmp_path_factory, gpu_ctx, poseidon):
    """A circuit directory: c.r1cs, c.zkwp, c_final.zkey, good.wtns, bad.wtns (wire 122 moved)"""
    from zkfl import wprog, zkey
    b, cons, w, _ = poseidon
    d = tmp_path_factory.mktemp("wchk")
    (d / "c.r1cs").write_bytes(b.r1cs_bytes())
    (d / "c.zkwp").write_bytes(wprog.compile_program(b))
    (d / "c_final.zkey").write_bytes(
        zkey.groth16_setup(b, gpu_ctx, zkey.Toxic(tau=31, alpha=3, beta=5, gamma=7, delta=11)))
    (d / "good.wtns").write_bytes(rs.wtns_of(w))
    (d / "bad.wtns").write_bytes(rs.wtns_of(_bump(w, 122)))
    (d / "input.json").write_text(json.dumps({"left": "1", "right": "2"}))
    return d, rs.expected(cons, _bump(w, 122))


def _assert_failure_lines(p, exp):
    n_failed, first, a, b, c = exp
    assert p.returncode == 1
    assert "[ERROR] snarkJS: WITNESS IS NOT CORRECT" in p.stderr
    assert f"first failing constraint: #{first}" in p.stderr
    for name, v in (("a", a), ("b", b), ("c", c)):
        assert f"{name} = {v}" in p.stderr
    assert f"{n_failed} of 241 constraints fail" in p.stderr


def test_cli_wtns_check(files):
    d, exp = files
    py = sys.executable
    p = _run(f"{py} -m zkfl wtns check c.r1cs good.wtns", d)
    assert "[INFO]  snarkJS: WITNESS IS CORRECT" in p.stdout
    _assert_failure_lines(_run(f"{py} -m zkfl wtns check c.r1cs bad.wtns", d, ok=False), exp)
    assert "WITNESS IS CORRECT" in _run(f"{py} -m zkfl wchk c.r1cs good.wtns", d).stdout
    assert _run(f"{py} -m zkfl wchk c.r1cs bad.wtns", d, ok=False).returncode == 1
    # the witness-generation subcommand of the same name still works
    _run(f"{py} -m zkfl wtns c.zkwp input.json made.wtns", d)
    assert (d / "made.wtns").read_bytes() == (d / "good.wtns").read_bytes()


def test_cli_prove_refuses_bad_witness(files):
    d, exp = files
    py = sys.executable
    p = _run(f"{py} -m zkfl prove c_final.zkey bad.wtns bad_proof.json bad_public.json --r1cs c.r1cs", d, ok=False)
    assert p.returncode == 1 and f"constraint #{exp[1]}" in p.stderr
    assert not (d / "bad_proof.json").exists() and not (d / "bad_public.json").exists()
    _run(f"{py} -m zkfl prove c_final.zkey good.wtns proof.json public.json --r1cs c.r1cs", d)
    assert json.load(open(d / "proof.json"))["protocol"] == "groth16"


def test_python_api(files, gpu_ctx):
    from zkfl import groth16, native
    d, exp = files
    assert groth16.wtns_check(str(d / "c.r1cs"), str(d / "good.wtns"), ctx=gpu_ctx) is True
    assert groth16.wtns_check((d / "c.r1cs").read_bytes(), (d / "bad.wtns").read_bytes(), ctx=gpu_ctx) is False
    rep = groth16.wtns_check_report(str(d / "c.r1cs"), str(d / "bad.wtns"), ctx=gpu_ctx)
    assert (rep.n_failed, rep.first, rep.a, rep.b, rep.c) == exp
    p = groth16.Prover(0)
    try:
        with pytest.raises(native.ZkflError) as e:
            p.prove(str(d / "c_final.zkey"), str(d / "bad.wtns"), r1cs=str(d / "c.r1cs"))
        assert e.value.code == E_CONSTRAINT
        proof, _ = p.prove(str(d / "c_final.zkey"), str(d / "good.wtns"), r1cs=str(d / "c.r1cs"))
        assert proof["protocol"] == "groth16"
    finally:
        p.close()


@pytest.mark.skipif(shutil.which("node") is None or shutil.which("npm") is None, reason="needs node")
def test_node_shim_wtns_check(files, tmp_path):
    """`npx snarkjs wtns check` / `wchk` and the module's wtns.check, resolved to this package
    (the harness of tests/test_gpu_node_dropin.py)."""
    d, exp = files
    (tmp_path / "package.json").write_text(json.dumps({"name": "harness", "version": "1.0.0", "private": True,
                                                       "dependencies": {"zkfl-snarkjs": "file:" + PKG}}))
    _run("npm install --offline --no-audit --no-fund", tmp_path)
    npx = f"{tmp_path}/node_modules/.bin/snarkjs"
    p = _run(f"{npx} wtns check {d}/c.r1cs {d}/good.wtns", tmp_path)
    assert "[INFO]  snarkJS: WITNESS IS CORRECT" in p.stdout
    _assert_failure_lines(_run(f"npx snarkjs wtns check {d}/c.r1cs {d}/bad.wtns", tmp_path, ok=False), exp)
    assert _run(f"npx snarkjs wchk {d}/c.r1cs {d}/bad.wtns", tmp_path, ok=False).returncode == 1
    (tmp_path / "api.js").write_text(f"""
const snarkjs = require('zkfl-snarkjs');
(async () => {{
  const good = await snarkjs.wtns.check({json.dumps(str(d / 'c.r1cs'))}, {json.dumps(str(d / 'good.wtns'))});
  const bad = await snarkjs.wtns.check({json.dumps(str(d / 'c.r1cs'))}, {json.dumps(str(d / 'bad.wtns'))});
  console.log(JSON.stringify({{ good, bad }}));
  process.exit(0);
}})().catch((e) => {{ console.error(e); process.exit(1); }});
""")
    p = _run("node api.js", tmp_path)
    assert json.loads(p.stdout.strip().splitlines()[-1]) == {"good": True, "bad": False}
