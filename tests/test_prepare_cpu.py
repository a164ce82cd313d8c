"""Round preparation on the host: the model against the circuits, pack's refusals, input_json, the CLI.

tests/prepare_model.py is what tests/test_gpu_prepare.py holds the device to, so it is checked here
against the three circuits themselves (oracle.witness.evaluate + check_all) at the shapes where the
arithmetic has an edge: negative sums that divide exactly and that do not, a leaf of 17 values,
zero-subtree siblings, ids at both ends of the unsigned 64-bit range.  zkfl/prepare.py's host half --
pack's refusals, input_json against zkfl/clients.py, `python -m zkfl prepare-round`'s exit code 2 -- needs
no GPU either.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import prepare_model as M
from oracle import witness as ow
from zkfl import circuits, clients, prepare
from zkfl.field import R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "verifiable-federated-training-with-zero-knowledge-proofs-zk-fl-_amd")
U64 = (1 << 64) - 1


def _satisfies(shape, inp):
    b = circuits.build(*shape)
    w = ow.evaluate(b, inp)
    assert b.check_all(w)


def _c7(samples, dim, depth, batch, weights, **kw):
    """One client, id 7, clients.Client(7, samples, dim, depth, JsLcg(12352))'s dataset."""
    return M.harness_spec([7], samples, dim, depth, batch, weights=weights, peers=False, **kw)


# (samples, batch, dim, depth, weights, expected gradient[0], expected remainder[0])
TRAINING = [
    (2, 2, 1, 1, [0], -14, 0),                 # a negative sum that divides exactly
    (2, 2, 1, 1, [-3], -18, 1973),             # negative, floor != truncation
    (5, 3, 16, 3, [(-1) ** j * (j + 1) for j in range(16)], None, None),  # leaf of 17 values, z_l siblings
    (1, 1, 4, 1, [5, -2, 0, 1], None, None),
    (5, 5, 4, 3, [0, 0, 0, 0], None, None),
    (2, 2, 1, 1, [40], None, None),            # a weight that makes the gradient positive
]


@pytest.mark.parametrize("samples,batch,dim,depth,weights,g0,r0", TRAINING)
def test_model_training_inputs_satisfy_the_circuit(samples, batch, dim, depth, weights, g0, r0):
    spec = _c7(samples, dim, depth, batch, weights)
    c = M.client(spec, 0)
    ref = clients.Client(7, samples, dim, depth, clients.JsLcg(12352))
    assert spec["features"][0] == ref.features and spec["labels"][0] == ref.labels
    assert int(c["training"]["root_D"]) == ref.root_D
    if g0 is not None:
        assert c["gradient"][0] == g0 and int(c["training"]["remainder"][0]) == r0
    if weights == [40]:
        assert c["gradient"][0] > 0
    shape = M.shapes(spec)["training"]
    # tau_squared = norm^2 passes, one less is refused: by the model's status and by the circuit
    spec["tau_squared"] = c["norm"]
    at = M.client(spec, 0)
    assert at["status"] == M.OK
    _satisfies(shape, at["training"])
    if c["norm"] > 0:
        spec["tau_squared"] = c["norm"] - 1
        below = M.client(spec, 0)
        assert below["status"] == M.NORM
        with pytest.raises(ow.AssertFailed):
            ow.evaluate(circuits.build(*shape), below["training"])


def test_model_balance_inputs_satisfy_the_circuit():
    spec = _c7(5, 4, 3, 5, [0] * 4)
    c = M.client(spec, 0)
    assert c["balance"] == clients.Client(7, 5, 4, 3, clients.JsLcg(12352)).balance_input()
    _satisfies(("balance_unified", 5, 3, 4), c["balance"])


def _secagg_spec(cid, peers, dim):
    spec = M.harness_spec([cid], 1, dim, 1, 1, peers=False, weights=[3] * dim)
    spec["features"], spec["labels"] = [[[(7 * k + 3) % 101 for k in range(dim)]]], [[1]]   # the LCG is for small ids
    spec["peers"] = [list(peers)]
    spec["keys"] = [[clients.shared_key(cid, p) for p in peers]]
    spec["master_keys"] = [clients.poseidon_hash([cid, 12345])]
    return spec


@pytest.mark.parametrize("dim,cid,peers", [
    (17, 5, [9]),
    (4, U64, list(range(U64 - 15, U64))),      # every peer sorts below the client
    (1, 0, [U64]),
    (4, 2, [1, 3]),
])
def test_model_secagg_inputs_satisfy_the_circuit(dim, cid, peers):
    spec = _secagg_spec(cid, peers, dim)
    c = M.client(spec, 0)
    assert c["norm"] > 0
    spec["tau_squared"] = c["norm"]
    at = M.client(spec, 0)
    shape = M.shapes(spec)["secagg"]
    _satisfies(shape, at["secagg"])
    assert at["secagg"]["root_D"] == at["training"]["root_D"] and at["secagg"]["root_G"] == at["training"]["root_G"]
    spec["tau_squared"] = c["norm"] - 1
    with pytest.raises(ow.AssertFailed):
        ow.evaluate(circuits.build(*shape), M.client(spec, 0)["secagg"])


# ---------------------------------------------------------------------------
# pack's refusals: one per rule of include/zkfl.h
# ---------------------------------------------------------------------------
def _spec(**over):
    spec = M.harness_spec([1, 2, 3], 3, 2, 2, 2)
    spec.update(over)
    return spec


def _refused(match, **over):
    with pytest.raises(ValueError, match=match):
        prepare.pack(_spec(**over))


def test_pack_accepts_the_harness_spec():
    a = prepare.pack(_spec())
    assert a["peers"] == 2 and a["features"].shape == (3, 3, 2) and a["keys"].shape == (3, 2, 32)
    assert prepare.pack(_spec(peers=None, keys=None, master_keys=None))["peers"] == 0


@pytest.mark.parametrize("dim", [0, 256])
def test_pack_refuses_dim(dim):
    _refused("dim", dim=dim, features=np.zeros((3, 3, dim), np.int64), weights=[0] * dim)


@pytest.mark.parametrize("depth", [0, 31])
def test_pack_refuses_depth(depth):
    _refused("depth", depth=depth)


def test_pack_refuses_samples():
    _refused("samples", samples=0)
    _refused("samples", samples=5)            # 2^depth = 4


def test_pack_refuses_batch():
    _refused("batch", batch=0)
    _refused("batch", batch=4)


def test_pack_refuses_batch_idx():
    _refused("client 1: batch_idx 1", batch_idx=[[0, 1], [2, 3], [0, 0]])


def test_pack_refuses_label():
    lab = [[0, 1, 0], [1, 0, 1], [0, 2, 0]]
    _refused("client 2: label 1", labels=lab)


def test_pack_refuses_precision_zero():
    _refused("precision", precision=0)


def test_pack_refuses_tau_all_ones():
    _refused("tau_squared", tau_squared=U64)
    prepare.pack(_spec(tau_squared=U64 - 1))


def test_pack_refuses_sixteen_peers():
    ids = list(range(1, 18))
    spec = M.harness_spec(ids, 1, 1, 1, 1, peers=False)
    spec["peers"] = [[p for p in ids if p != c] for c in ids]
    spec["keys"] = [[1] * 16 for _ in ids]
    spec["master_keys"] = [1] * 17
    with pytest.raises(ValueError, match="peers 16"):
        prepare.pack(spec)


def test_pack_refuses_keys_without_peers():
    _refused("peers == 0", peers=None)
    _refused("peers == 0", peers=[[], [], []])


def test_pack_refuses_own_id_and_repeated_peer():
    _refused("client 1: peer 0 is the client's own id", peers=[[2, 3], [2, 3], [1, 2]])
    _refused("client 2: peer 1 repeats peer 0", peers=[[2, 3], [1, 3], [1, 1]])


def test_pack_refuses_values_not_below_r():
    keys = _spec()["keys"]
    keys[1][1] = R
    _refused("client 1: key 1", keys=keys)
    _refused("client 2: master key", master_keys=[1, 2, R])
    _refused("round", round=R)


def test_pack_overflow_bound_one_below_and_one_above():
    # dim 1, batch 1, precision 1, one sample: the bound is F * (F * W + 1)
    def spec(F, W):
        return {"ids": [1], "samples": 1, "dim": 1, "depth": 1, "batch": 1, "precision": 1, "features": [[[F]]],
                "labels": [[0]], "weights": [W], "round": 1, "tau_squared": 1}
    F = 3037000499                              # floor(sqrt(2^63 - 1))
    W = ((1 << 63) - 1) // (F * F)              # 1
    assert F * (F * W + 1) <= (1 << 63) - 1 < (F + 1) * ((F + 1) * W + 1)
    prepare.pack(spec(F, W))
    prepare.pack(spec(-F, -W))
    with pytest.raises(ValueError, match="overflow bound"):
        prepare.pack(spec(F + 1, W))
    # exactly at the limit, and one above it
    lim = (1 << 63) - 1
    prepare.pack(spec(lim, 0))                  # F * (0 + 1) = 2^63 - 1
    with pytest.raises(ValueError, match="overflow bound"):
        prepare.pack(spec(-(1 << 63), 0))       # |F| = 2^63


def test_pack_harness_values_are_far_inside_the_bound():
    a = prepare.pack(M.harness_spec(range(1, 9), 8, 4, 3, 8))
    assert 8 * 100 * (4 * 100 * 0 + 1000) < 1 << 20 and int(a["features"].max()) <= 100


# ---------------------------------------------------------------------------
# input_json against zkfl/clients.py, at the harness's defaults
# ---------------------------------------------------------------------------
def test_input_json_equals_clients_py_at_the_harness_defaults():
    ids = [1, 2, 3]
    spec = M.harness_spec(ids, 8, 4, 3, 8)
    res = prepare.Prepared(prepare.pack(spec), M.result(spec))
    fed = clients.federated_round(n_clients=3)
    for i, cid in enumerate(ids):
        c = clients.Client(cid, 8, 4, 3, clients.JsLcg(12345 + cid))
        assert res.input_json("balance", i) == c.balance_input()
        tr, grad = c.training_input(8, 1000, 100000000)
        assert res.input_json("training", i) == tr == fed[i][0]
        assert res.input_json("secagg", i) == fed[i][1]
        assert [int(x) for x in res.gradients[i]] == grad
    assert res.ok
    # the package fields admit.pack reads
    rnd = res.round({}, {})
    assert rnd["clients"] == ids and rnd["peers"][2] == [1, 3] and rnd["weights"] == [0, 0, 0, 0]


def test_input_json_keeps_signed_weights_and_batch_rows():
    spec = M.harness_spec([4, 9], 5, 3, 3, 2, weights=[2, -1, 0])
    spec["batch_idx"] = [[4, 4], [3, 0]]
    cl = [M.client(spec, i) for i in range(2)]
    res = prepare.Prepared(prepare.pack(spec), M.result(spec, cl))
    for i in range(2):
        for phase in prepare.PHASES:
            assert res.input_json(phase, i) == cl[i][phase]


# ---------------------------------------------------------------------------
# the command line: exit 2 before the GPU is touched
# ---------------------------------------------------------------------------
def _cli(*args):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT)
    return subprocess.run([sys.executable, "-m", "zkfl", *args], env=env, capture_output=True, text=True, timeout=120)


def test_cli_prepare_round_exit_2(tmp_path):
    out = tmp_path / "out"
    assert _cli("prepare-round", str(tmp_path / "missing.json"), "-o", str(out)).returncode == 2
    man = tmp_path / "m.json"
    man.write_text(json.dumps([1, 2]))
    assert _cli("prepare-round", str(man), "-o", str(out)).returncode == 2
    good = {"round": 1, "tau_squared": 100000000, "depth": 1, "batch": 2, "precision": 1000, "weights": [0, 0],
            "clients": [{"id": 1, "features": [[1, 2], [3, 4]], "labels": [0, 1]}]}
    for key, value, needle in (("precision", 0, "precision"), ("batch", 3, "batch"), ("tau_squared", U64, "tau_squared")):
        man.write_text(json.dumps(dict(good, **{key: value})))
        r = _cli("prepare-round", str(man), "-o", str(out))
        assert r.returncode == 2 and needle in r.stderr, r.stderr
    bad_label = dict(good, clients=[dict(good["clients"][0], labels=[0, 2])])
    man.write_text(json.dumps(bad_label))
    r = _cli("prepare-round", str(man), "-o", str(out))
    assert r.returncode == 2 and "client 0: label 1" in r.stderr
    assert not out.exists()
