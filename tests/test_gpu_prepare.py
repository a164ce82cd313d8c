"""Preparing a round on the GPU (zkfl_round_prepare; csrc/prepare.hip) — MI355X.

Bar: byte equality of every output with tests/prepare_model.py, the plain-Python restatement built
from zkfl/clients.py (itself held to the circuits in tests/test_prepare_cpu.py).  Shapes: the edge cases
of the CPU file, every path of the leaf hash (one Poseidon up to 16 values, chunks above), full and
ragged trees, chosen batch rows, every nullable output.  Sizes: around a wave and a workgroup.  Then
the status, the launch count, the witness engine on the prepared vectors, and the chain from a dataset
to the aggregate at the smallest shape.  The model's Python Poseidon is the cost, so shapes stay small
and each model result is computed once.
"""
import functools
import types

import numpy as np
import pytest

import prepare_model as M
from zkfl import admit, circuits, clients, native, prepare, secagg, wprog

pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1
PROFILED = ("prepare_leaves", "prepare_levels", "prepare_open", "prepare_gradient", "prepare_commit",
            "prepare_masks", "prepare_inputs")


def ring_spec(n, samples, dim, depth, batch, peers, weights=None, first_id=1, **kw):
    """n harness clients; client i's peers are the next `peers` ids round the ring (prepare does not
    need the lists to be symmetric), keys the harness's."""
    ids = list(range(first_id, first_id + n))
    spec = M.harness_spec(ids, samples, dim, depth, batch, weights=weights, peers=False, **kw)
    if peers:
        spec["peers"] = [[ids[(i + 1 + j) % n] for j in range(peers)] for i in range(n)]
        spec["keys"] = [[clients.shared_key(c, p) for p in lst] for c, lst in zip(ids, spec["peers"])]
        spec["master_keys"] = [clients.poseidon_hash([c, 12345]) for c in ids]
    return spec


def _alt(dim):
    return [(-1) ** j * (j + 1) for j in range(dim)]


def _secagg_edge(cid, peers, dim):
    spec = M.harness_spec([cid], 1, dim, 1, 1, peers=False, weights=[3] * dim)
    spec["features"], spec["labels"] = [[[(7 * k + 3) % 101 for k in range(dim)]]], [[1]]
    spec["peers"] = [list(peers)]
    spec["keys"] = [[clients.shared_key(cid, p) for p in peers]]
    spec["master_keys"] = [clients.poseidon_hash([cid, 12345])]
    return spec


def _with_rows(spec, rows):
    spec["batch_idx"] = rows
    return spec


# name -> spec; every one is a shape at which the device code takes another path
CASES = {
    # the CPU file's shapes (id 7, JsLcg(12352))
    "neg_exact": lambda: M.harness_spec([7], 2, 1, 1, 2, weights=[0], peers=False),
    "neg_floor": lambda: M.harness_spec([7], 2, 1, 1, 2, weights=[-3], peers=False),
    "leaf17_zero_siblings": lambda: M.harness_spec([7], 5, 16, 3, 3, weights=_alt(16), peers=False),
    "one_sample": lambda: M.harness_spec([7], 1, 4, 1, 1, weights=[5, -2, 0, 1], peers=False),
    "zeros_w": lambda: M.harness_spec([7], 5, 4, 3, 5, peers=False),
    "positive_gradient": lambda: M.harness_spec([7], 2, 1, 1, 2, weights=[40], peers=False),
    "secagg_17_1": lambda: _secagg_edge(5, [9], 17),
    "secagg_15_peers_top_id": lambda: _secagg_edge(U64, list(range(U64 - 15, U64)), 4),
    "secagg_id0_peer_top": lambda: _secagg_edge(0, [U64], 1),
    "secagg_4_2": lambda: _secagg_edge(2, [1, 3], 4),
    # the leaf hash: 16 values in one Poseidon of width 17; 34 values in three chunks
    "dim15": lambda: ring_spec(2, 3, 15, 2, 2, 1, weights=_alt(15)),
    "dim33": lambda: ring_spec(2, 2, 33, 1, 2, 1, weights=_alt(33)),
    # the tree: samples = 2^depth exactly; an odd count whose last leaf pairs with z_0
    "full_tree": lambda: ring_spec(3, 4, 2, 2, 4, 2),
    "odd_last_leaf": lambda: ring_spec(3, 5, 2, 3, 5, 2),
    # batch rows: the last leaf and a repeated index; a permutation
    "rows_last_repeated": lambda: _with_rows(ring_spec(2, 5, 3, 3, 3, 1, weights=[2, -1, 0]), [[4, 4, 0], [2, 4, 4]]),
    "rows_permutation": lambda: _with_rows(ring_spec(2, 4, 2, 2, 4, 1, weights=[1, 1]), [[3, 1, 0, 2], [1, 0, 3, 2]]),
    # sizes: one, a few, one more than a wave -- with one hash per leaf and with the chunk pass
    "n1_dim1": lambda: ring_spec(1, 2, 1, 1, 2, 0, weights=[-3]),
    "n3_dim1": lambda: ring_spec(3, 2, 1, 1, 2, 2, weights=[-3]),
    "n65_dim1": lambda: ring_spec(65, 2, 1, 1, 2, 2, weights=[-3]),
    "n1_dim17": lambda: ring_spec(1, 2, 17, 1, 1, 0, weights=_alt(17)),
    "n3_dim17": lambda: ring_spec(3, 2, 17, 1, 1, 1, weights=_alt(17)),
    "n65_dim17": lambda: ring_spec(65, 2, 17, 1, 1, 1, weights=_alt(17)),
    # one more than a workgroup in every kernel, (client, node) indexing at the top levels included
    "n257": lambda: ring_spec(257, 3, 1, 2, 2, 1, weights=[7]),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(spec, the model's per-client results, the model's arrays): computed once, never changed."""
    spec = CASES[name]()
    cl = [M.client(spec, i) for i in range(len(spec["ids"]))]
    return spec, cl, M.result(spec, cl)


def _equal(got, want, what=""):
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k)
        assert np.array_equal(got[k], want[k]), (what, k, np.argwhere(got[k] != want[k])[:4].tolist())


@pytest.mark.parametrize("name", list(CASES))
def test_every_output_equals_the_model(gpu_ctx, name):
    spec, _, want = case(name)
    _equal(gpu_ctx.round_prepare(prepare.pack(spec)), want, name)


def test_each_nullable_output_null_in_turn(gpu_ctx):
    spec, _, want = case("odd_last_leaf")
    a = prepare.pack(spec)
    for skip in native.PREPARE_OUTPUTS:
        names = [k for k in native.PREPARE_OUTPUTS if k != skip]
        _equal(gpu_ctx.round_prepare(a, names), {k: want[k] for k in names}, skip)
    for only in native.PREPARE_OUTPUTS:
        _equal(gpu_ctx.round_prepare(a, [only]), {only: want[only]}, only)
    assert gpu_ctx.round_prepare(a, []) == {}


def test_no_peers_means_no_secagg_part(gpu_ctx):
    spec, _, want = case("zeros_w")
    got = gpu_ctx.round_prepare(prepare.pack(spec))
    assert "secagg_inputs" not in got and "masked" not in got
    assert not got["roots"][:, 3].any()                      # root_K reads zero without keys
    _equal(got, want)


# ---------------------------------------------------------------------------
# status
# ---------------------------------------------------------------------------
def test_status_at_the_bound_below_it_and_mixed(gpu_ctx):
    spec, cl, _ = case("full_tree")
    norms = [c["norm"] for c in cl]
    assert len(set(norms)) > 1 and min(norms) > 0
    for tau, expect in ((max(norms), [0] * 3), (min(norms) - 1, [1] * 3),
                        (min(norms), [int(x > min(norms)) for x in norms])):
        s = dict(spec, tau_squared=tau)
        per = [M.client(s, i) for i in range(3)]
        assert [c["status"] for c in per] == expect
        got = gpu_ctx.round_prepare(prepare.pack(s))
        assert got["status"].tolist() == expect
        _equal(got, M.result(s, per), tau)                   # a NORM client's inputs are still the model's
    assert 0 < sum(int(x > min(norms)) for x in norms) < 3   # honest and clipped clients in one call
    # exactly at each client's own norm
    for i, nrm in enumerate(norms):
        got = gpu_ctx.round_prepare(prepare.pack(dict(spec, tau_squared=nrm)), ["status"])["status"]
        assert got[i] == 0 and got.tolist() == [int(x > nrm) for x in norms]


def test_norm_saturates_instead_of_wrapping(gpu_ctx):
    """|g| = 2^32 squares to 2^64: a wrapped norm would read 0 and pass any tau."""
    spec = {"ids": [1], "samples": 1, "dim": 2, "depth": 1, "batch": 1, "precision": 1,
            "features": [[[1 << 16, 1]]], "labels": [[0]], "weights": [1 << 16, 0], "round": 1, "tau_squared": U64 - 1}
    grad, _, _ = M.gradient(spec["features"][0], [0], [0], spec["weights"], 1)
    assert grad == [1 << 48, 1 << 32] and sum(g * g for g in grad) > U64
    got = gpu_ctx.round_prepare(prepare.pack(spec), ["status", "gradients"])
    assert got["gradients"].tolist() == [grad] and got["status"].tolist() == [native.PREPARE_NORM]


# ---------------------------------------------------------------------------
# launches do not depend on n
# ---------------------------------------------------------------------------
def _launches(ctx, spec):
    ctx.set_profiling(True)
    try:
        ctx.profile_reset()
        ctx.round_prepare(prepare.pack(spec))
        ctx.synchronize()
        counts = {k: ctx.profile(k)[1] for k in PROFILED}
        ctx.profile_reset()
    finally:
        ctx.set_profiling(False)
    return counts


def test_launch_count_is_the_same_for_3_and_65_clients(gpu_ctx):
    small, large = _launches(gpu_ctx, case("n3_dim17")[0]), _launches(gpu_ctx, case("n65_dim17")[0])
    assert small == large and sum(small.values()) == 7 and all(small.values())
    assert _launches(gpu_ctx, case("odd_last_leaf")[0])["prepare_levels"] == 3     # one per tree level


# ---------------------------------------------------------------------------
# the witness engine takes the vectors as they are
# ---------------------------------------------------------------------------
def test_witness_engine_accepts_ok_clients_and_refuses_a_norm_client(gpu_ctx):
    spec, cl, _ = case("full_tree")
    norms = [c["norm"] for c in cl]
    s = dict(spec, tau_squared=min(norms))
    res = prepare.prepare_round(gpu_ctx, s)
    ok = [i for i in range(3) if res.status[i] == 0]
    clipped = [i for i in range(3) if res.status[i] != 0]
    assert ok and clipped
    for phase, shape in M.shapes(s).items():
        b = circuits.build(*shape)
        wp = native.WitnessProgram(gpu_ctx, wprog.compile_program(b))
        try:
            rows = res.inputs[phase]
            want = (ok if phase != "balance" else range(3))           # balance does not look at the gradient
            wt = wp.compute([rows[i] for i in want])
            assert len(wt) == len(want)
            if phase != "balance":
                with pytest.raises(native.ZkflError) as e:
                    wp.compute([rows[clipped[0]]])
                assert e.value.code == -7                             # ZKFL_E_CONSTRAINT
        finally:
            wp.close()


# ---------------------------------------------------------------------------
# the chain at the smallest shape: dataset -> prepare -> prove -> admit -> aggregate
# ---------------------------------------------------------------------------
def test_chain_prepare_prove_admit_aggregate(gpu_ctx):
    from zkfl import groth16, zkey
    ids = [1, 2, 3]
    data = [prepare.harness_dataset(c, 2, 4) for c in ids]
    spec = {"ids": ids, "samples": 2, "dim": 4, "depth": 1, "batch": 2, "precision": 1000,
            "features": [f for f, _ in data], "labels": [l for _, l in data], "weights": [0, 0, 0, 0],
            "round": 1, "tau_squared": 100000000}
    spec["peers"], spec["keys"], spec["master_keys"] = prepare.harness_keys(ids)
    res = prepare.prepare_round(gpu_ctx, spec)
    assert res.ok
    shapes = {"balance": ("balance_unified", 2, 1, 4), "training": ("sgd_verified", 2, 4, 1, 1000),
              "secagg": ("secure_masked_update", 4, 2)}
    assert M.shapes(spec) == shapes
    proofs, vkeys = {}, {}
    try:
        for seed, (phase, shape) in enumerate(shapes.items()):
            b = circuits.build(*shape)
            s = 0xAD0 + 16 * seed
            zk = zkey.groth16_setup(b, gpu_ctx, zkey.Toxic(tau=s, alpha=s + 1, beta=s + 2, gamma=s + 3, delta=s + 4))
            key = native.ProvingKey(gpu_ctx, zk)
            wp = native.WitnessProgram(gpu_ctx, wprog.compile_program(b))
            proofs[phase] = key.full_prove_batch(wp, res.inputs[phase])
            wp.close()
            key.close()
            vkeys[phase] = native.VerifyingKey(gpu_ctx, groth16.vk_bytes(groth16.export_verification_key(zk, alphabeta=False)))
        rnd = res.round(proofs, vkeys)
        adm = admit.admit_round(types.SimpleNamespace(ctx=gpu_ctx), rnd)     # all checks on
        assert adm.codes == {c: (0, 0, 0) for c in ids}
    finally:
        for k in vkeys.values():
            k.close()
    out = secagg.close_groups(gpu_ctx, [{"roster": ids, "accepted": {c: rnd["secagg"][c]["masked_update"] for c in ids},
                                         "revealed": []}], 1)
    assert out[0]["sum"] == res.gradients.sum(axis=0).tolist() and not out[0]["out_of_range"]
    assert any(out[0]["sum"])


# ---------------------------------------------------------------------------
# argument errors through the C ABI, the message naming the index
# ---------------------------------------------------------------------------
def _packed(**over):
    a = prepare.pack(case("full_tree")[0])
    a.update(over)
    return a


def _arg_error(ctx, match, want=None, **over):
    with pytest.raises(native.ZkflError, match=match) as e:
        ctx.round_prepare(_packed(**over), want)
    assert e.value.code == -1, e.value


def test_argument_errors(gpu_ctx):
    ctx = gpu_ctx
    a = _packed()
    n, S, dim = 3, 4, 2
    _arg_error(ctx, "dim 0", dim=0, features=np.zeros(0, np.int64), weights=np.zeros(0, np.int64))
    _arg_error(ctx, "dim 256", dim=256, features=np.zeros(n * S * 256, np.int64), weights=np.zeros(256, np.int64))
    _arg_error(ctx, "depth 0", depth=0)
    _arg_error(ctx, "depth 31", depth=31)
    _arg_error(ctx, "samples 0", samples=0, features=np.zeros(0, np.int64), labels=np.zeros(0, np.uint8))
    _arg_error(ctx, "samples 5", samples=5, features=np.zeros(n * 5 * dim, np.int64), labels=np.zeros(n * 5, np.uint8))
    _arg_error(ctx, "batch 0", batch=0)
    _arg_error(ctx, "batch 5", batch=5)
    idx = np.tile(np.arange(4, dtype=np.uint32), (3, 1))
    idx[2, 1] = 4
    _arg_error(ctx, "client 2: batch_idx 1 is 4", batch_idx=idx)
    lab = a["labels"].copy()
    lab[1, 3] = 2
    _arg_error(ctx, "client 1: label 3 is 2", labels=lab)
    _arg_error(ctx, "precision", precision=0)
    _arg_error(ctx, "tau_squared", tau_squared=U64)
    _arg_error(ctx, "peers 16", peers=16, peer_ids=np.zeros(n * 16, np.uint64), keys=np.zeros(n * 16 * 32, np.uint8))
    # peers == 0 with any secagg output or input
    none = dict(peers=0, peer_ids=None, keys=None, master_keys=None)
    _arg_error(ctx, "peers == 0", **dict(none, master_keys=a["master_keys"]))
    _arg_error(ctx, "peers == 0", ["secagg_inputs"], **none)
    _arg_error(ctx, "peers == 0", ["masked"], **none)
    assert set(ctx.round_prepare(_packed(**none), ["roots", "status"])) == {"roots", "status"}
    pid = a["peer_ids"].copy()
    pid[1, 0] = a["ids"][1]
    _arg_error(ctx, "client 1: peer 0 is the client's own id", peer_ids=pid)
    pid = a["peer_ids"].copy()
    pid[2, 1] = pid[2, 0]
    _arg_error(ctx, "client 2: peer 1 repeats peer 0", peer_ids=pid)
    r_bytes = np.frombuffer(M.R.to_bytes(32, "little"), dtype=np.uint8)
    keys = a["keys"].copy()
    keys[1, 1] = r_bytes
    _arg_error(ctx, "client 1: key 1 is not < r", keys=keys)
    mk = a["master_keys"].copy()
    mk[2] = r_bytes
    _arg_error(ctx, "client 2: master key is not < r", master_keys=mk)
    _arg_error(ctx, "round is not < r", round=M.R)
    # the overflow bound: |feature| = 2^32 with weight 2^31 at dim 2, batch 4 is past 2^63 - 1
    f = a["features"].copy()
    f[1, 2, 0] = -(1 << 32)
    _arg_error(ctx, r"overflow bound.*client 1, feature 4", features=f, weights=np.array([1 << 31, 0], np.int64))


def test_overflow_bound_one_below_and_one_above_through_the_abi(gpu_ctx):
    def spec(F, W):
        return {"ids": np.array([1], np.uint64), "samples": 1, "dim": 1, "depth": 1, "batch": 1, "precision": 1,
                "peers": 0, "features": np.array([F], np.int64), "labels": np.zeros(1, np.uint8),
                "weights": np.array([W], np.int64), "round": 1, "tau_squared": 1, "batch_idx": None}
    lim = (1 << 63) - 1
    got = gpu_ctx.round_prepare(spec(lim, 0), ["gradients", "status"])     # F * (0 + 1) = 2^63 - 1: label 0, sum 0
    assert got["gradients"].tolist() == [[0]] and got["status"].tolist() == [0]
    F = 3037000499                                                        # F * (F + 1) <= 2^63 - 1 < (F + 1) * (F + 2)
    assert F * (F + 1) <= lim < (F + 1) * (F + 2)
    got = gpu_ctx.round_prepare(spec(F, 1), ["gradients", "status"])      # summed = (F * 1 - 0) * F
    assert got["gradients"].tolist() == [[F * F]] and got["status"].tolist() == [1]
    for bad in (spec(-(1 << 63), 0), spec(F + 1, 1)):
        with pytest.raises(native.ZkflError, match="overflow bound") as e:
            gpu_ctx.round_prepare(bad)
        assert e.value.code == -1


def test_no_clients_is_valid(gpu_ctx):
    a = prepare.pack(dict(case("full_tree")[0], ids=[], features=np.zeros((0, 4, 2), np.int64),
                          labels=np.zeros((0, 4), np.uint8), peers=None, keys=None, master_keys=None))
    got = gpu_ctx.round_prepare(a)
    assert got["status"].shape == (0,) and got["training_inputs"].shape[0] == 0
