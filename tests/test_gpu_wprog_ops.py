"""GPU witness engine, opcode by opcode, vs the oracle -- MI355X.

tests/test_gpu_witness.py runs csrc/witness.hip on the five reference circuits with honest inputs,
which never execute K_INV (and with it the crossing into the 32-bit field engine), Poseidon widths
2, 7..16 (pos_rounds<3>, pos_rounds<4>), a live-S-box bitmap with holes past word 0, K_BITS above
129 bits or near r, the edge shapes of lc_eval, or a level with every kind of segment.  The synthetic
systems of tests/wprog_systems.py do.

Bar: bit-exact, every wire of every witness, against oracle/witness.py; a violated assert fails with
ZKFL_E_CONSTRAINT naming the lowest failing witness and its lowest failing assert; a circuit made
of the new ops proves bit-exactly and passes the R1CS check.
"""
import re

import pytest

from oracle import groth16 as og

import wprog_systems as ws

pytestmark = pytest.mark.gpu


def _prog(gpu_ctx, b):
    from zkfl import native, wprog
    return native.WitnessProgram(gpu_ctx, wprog.compile_program(b))


def _compute(gpu_ctx, name, count=None):
    """The system's inputs (the first `count`) in ONE call -> [wire tuple] per witness."""
    from zkfl import wprog, zkey
    b, inputs = ws.system(name)
    wp = _prog(gpu_ctx, b)
    try:
        got = wp.compute([wprog.input_bytes(b, x) for x in inputs[:count]])
    finally:
        wp.close()
    return [tuple(zkey.read_wtns(wt)) for wt in got]


def _assert_wires(name, got, want):
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        bad = [i for i in range(len(w)) if g[i] != w[i]]
        assert not bad, f"{name}: witness {j}: {len(bad)} of {len(w)} wires differ, first at wire {bad[0]}"
        assert g == w


@pytest.mark.parametrize("name", ws.NAMES)
def test_wires_match_oracle(gpu_ctx, name):
    _assert_wires(name, _compute(gpu_ctx, name), ws.reference(name))


def test_mixed_level_single_witness(gpu_ctx):
    """One witness: every segment of the level is a partial wave or a single block."""
    _assert_wires("mixed_level", _compute(gpu_ctx, "mixed_level", 1), ws.reference("mixed_level")[:1])


@pytest.mark.parametrize("name", ws.FAIL_NAMES)
def test_failure_names_lowest_witness_and_assert(gpu_ctx, name):
    """The engine numbers asserts by position in b.asserts; the oracle's AssertFailed names the
    index into b.cons (ws.first_failure maps one to the other)."""
    from zkfl import native, wprog
    b, inputs = ws.system(name)
    witness, a = ws.first_failure(name)
    wp = _prog(gpu_ctx, b)
    try:
        with pytest.raises(native.ZkflError) as e:
            wp.compute([wprog.input_bytes(b, x) for x in inputs])
    finally:
        wp.close()
    assert e.value.code == -7
    m = re.search(r"witness (\d+): assert constraint #(\d+) failed", str(e.value))
    assert m, str(e.value)
    assert (int(m.group(1)), int(m.group(2))) == (witness, a)


def test_new_ops_prove_and_check_end_to_end(gpu_ctx):
    """IsZero + Num2Bits(254) + Poseidon(8) from inputs to proof bytes: GPU witness (resident) ->
    GPU proof == the oracle's proof of the oracle's witness, and the resident witness satisfies the
    circuit's .r1cs on the GPU (csrc/r1cs_check.hip)."""
    from zkfl import native, wprog, zkey
    b, inputs = ws.system("e2e")
    want = ws.reference("e2e")
    zk = zkey.groth16_setup(b, gpu_ctx, zkey.Toxic(tau=77, alpha=2, beta=3, gamma=5, delta=7))
    key = native.ProvingKey(gpu_ctx, zk)
    wp = _prog(gpu_ctx, b)
    cs = native.R1cs(gpu_ctx, b.r1cs_bytes())
    res = wp.compute_resident(key, [wprog.input_bytes(b, x) for x in inputs])
    try:
        rs = (11).to_bytes(32, "little") + (13).to_bytes(32, "little")
        ref = og.prove(og.parse_zkey(zk), list(want[0]), r=11, s=13)
        assert key.prove_resident(res[0], rs) == og.proof_bytes(ref)
        reports = cs.check_resident(res)
        assert [r.ok for r in reports] == [True] * len(inputs), cs.last_error
    finally:
        for r_ in res:
            r_.close()
        cs.close()
        wp.close()
        key.close()
