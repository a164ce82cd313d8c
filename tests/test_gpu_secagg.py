"""GPU secure aggregation (zkfl_secagg_mask, zkfl_secagg_aggregate; csrc/secagg.hip) — MI355X.

Every oracle-checked case compares the library's bytes with the model of tests/secagg_model.py
(oracle/poseidon.py), which caches a pair's mask, so one case costs at most a few hundred CPU hashes.
The property case uses no oracle: whatever the masks are, they must cancel.
"""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from zkfl import clients, native, secagg
from zkfl.field import R

import secagg_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(native.LIB_PATH)
RND = 4


def _keys(seed, n):
    rng = random.Random(seed)
    return [rng.randrange(R) for _ in range(n)]


def _model_bytes(ids, peers, keys, rnd, grads):
    return M.fr_bytes([M.mask(i, p, k, rnd, g) for i, p, k, g in zip(ids, peers, keys, grads)])


def test_mask_parity_with_the_model_and_clients_py(gpu_ctx):
    ids = [1, 2, 3, 5, 9]
    grads = [[0, R - 7, R - 1], [1, 2, 3], [R - 1, 0, 10 ** 6], [R - 123456, 7, 0], [5, R - 5, 1 << 62]]
    peers = [[p for p in ids if p != i] for i in ids]
    inputs = [clients.secagg_input(i, p, g, RND, 10 ** 8, 1, 2) for i, p, g in zip(ids, peers, grads)]
    keys = [[int(k) for k in inp["shared_keys"]] for inp in inputs]
    got = secagg.mask_updates(gpu_ctx, ids, peers, keys, RND, grads)
    assert got.shape == (5, 3, 32)
    assert got.tobytes() == _model_bytes(ids, peers, keys, RND, grads)
    assert [[str(v) for v in row] for row in secagg.fr_ints(got)] == [inp["masked_update"] for inp in inputs]


def test_ids_compare_as_unsigned_64_bit_integers(gpu_ctx):
    """A 32-bit compare calls 2^32 smaller than 7 and 2^32 - 1; a signed one calls 2^64 - 1 negative:
    either gets a sign or a min / max wrong."""
    ids = [7, (1 << 32) - 1, 1 << 32, (1 << 64) - 1]
    peers = [[p for p in ids if p != i] for i in ids]
    pair_key = {frozenset(p): k for p, k in zip([(a, b) for a in ids for b in ids if a < b], _keys(2, 6))}
    keys = [[pair_key[frozenset((i, p))] for p in ps] for i, ps in zip(ids, peers)]
    grads = [[3], [R - 4], [0], [1 << 60]]
    got = secagg.mask_updates(gpu_ctx, ids, peers, keys, RND, grads)
    assert got.tobytes() == _model_bytes(ids, peers, keys, RND, grads)
    # and the four updates, every pair inside, sum to the gradients
    total = M.aggregate(secagg.fr_ints(got), [], RND)
    assert [M.signed(v) for v in total] == [(1 << 60) - 1]


RAGGED = dict(ids=[10, 11, 12], peers=[[], [20], [3, 40]], keys=[[], _keys(3, 1), _keys(4, 2)],
              grads=[[R - 1, 5], [0, 1], [2, R - 2]])


def test_ragged_rows_in_one_call(gpu_ctx):
    a = RAGGED
    got = secagg.mask_updates(gpu_ctx, a["ids"], a["peers"], a["keys"], RND, a["grads"])
    assert got.tobytes() == _model_bytes(a["ids"], a["peers"], a["keys"], RND, a["grads"])
    assert got[0].tobytes() == M.fr_bytes(a["grads"][0])            # no peers: the gradient itself


@pytest.mark.parametrize("dim,n_peers", [(65, 2), (257, 1)])
def test_lane_wave_and_block_edges_in_k(gpu_ctx, dim, n_peers):
    """dim 65: a wave's lanes straddle two chunks and the last wave is partly filled; dim 257: one lane
    into a second workgroup."""
    peers = [[50, 3][:n_peers]]
    keys = [_keys(dim, n_peers)]
    grads = [[(k * k) % 11 for k in range(dim)]]
    got = secagg.mask_updates(gpu_ctx, [9], peers, keys, RND, grads, chunk_terms=1)
    assert got.tobytes() == _model_bytes([9], peers, keys, RND, grads)


def test_every_chunk_length_gives_the_same_bytes(gpu_ctx):
    peers = [[1, 2, 3, 40, 50, 60, 70]]
    keys = [_keys(5, 7)]
    grads = [[R - 9, 9]]
    want = _model_bytes([8], peers, keys, RND, grads)
    for chunk in (1, 2, 3, 7, 8, 0):
        assert secagg.mask_updates(gpu_ctx, [8], peers, keys, RND, grads, chunk_terms=chunk).tobytes() == want, chunk


@pytest.fixture(scope="module")
def two_groups():
    """Group A: a roster of 6 with the lowest and the highest id excluded (both signs occur among
    its pairs); group B: nobody excluded.  dim 3, masked by the model."""
    rng = random.Random(6)
    rosters = [[11, 12, 13, 14, 15, 16], [21, 22, 23]]
    excluded = [{11, 16}, set()]
    groups, want = [], []
    for roster, out in zip(rosters, excluded):
        key = {frozenset((a, b)): rng.randrange(R) for a in roster for b in roster if a < b}
        grads = {i: [rng.randrange(-10 ** 6, 10 ** 6) for _ in range(3)] for i in roster}
        masked = {i: M.mask(i, [p for p in roster if p != i], [key[frozenset((i, p))] for p in roster if p != i],
                            RND, grads[i]) for i in roster}
        inc = [i for i in roster if i not in out]
        groups.append({"roster": roster, "accepted": {i: masked[i] for i in inc},
                       "revealed": [(i, j, key[frozenset((i, j))]) for i in inc for j in sorted(out)]})
        want.append([sum(grads[i][k] for i in inc) for k in range(3)])
    return groups, want


def test_aggregate_parity_and_the_out_of_range_tripwire(gpu_ctx, two_groups):
    groups, want = two_groups
    got = secagg.close_groups(gpu_ctx, groups, RND)
    for g, grp in enumerate(groups):
        model = M.aggregate(list(grp["accepted"].values()), grp["revealed"], RND)
        assert M.fr_bytes(got[g]["field"]) == M.fr_bytes(model)
        assert got[g]["sum"] == want[g] == M.decode(model)[0] and not got[g]["out_of_range"]
        assert got[g]["clients"] == len(grp["accepted"])
    # the same call with group A's pairs withheld (below close_groups, which would refuse it)
    masked = secagg.fr_bytes([u for grp in groups for u in grp["accepted"].values()])
    sums, sg, oor = gpu_ctx.secagg_aggregate([0, 4, 7], masked, [0, 0, 0], [], [], b"", RND, 3)
    assert list(oor) == [True, False]
    assert sg.tolist() == [[0, 0, 0], want[1]]
    assert sums[0].tobytes() == M.fr_bytes(M.aggregate(list(groups[0]["accepted"].values()), [], RND))
    assert sums[1].tobytes() == M.fr_bytes([v % R for v in want[1]])


def test_masks_cancel_at_a_size_with_many_workgroups(gpu_ctx):
    """64 clients in 4 groups of 16, dim 16, the harness's keys: no oracle, the masks must cancel."""
    rng = np.random.default_rng(7)
    ids = np.arange(1000, 1064, dtype=np.uint64)
    grads = rng.integers(-10 ** 6, 10 ** 6, size=(64, 16), dtype=np.int64)
    masked = secagg.round_masked_updates(gpu_ctx, ids, grads, RND, group_size=16)
    assert masked.shape == (64, 16, 32)
    assert not (masked[:, :, 8:] == 0).all()                                   # masked: field-sized values
    rosters = [[int(i) for i in ids[16 * g:16 * g + 16]] for g in range(4)]
    index = {int(i): n for n, i in enumerate(ids)}
    full = [{"roster": r, "accepted": {i: masked[index[i]] for i in r}, "revealed": []} for r in rosters]
    for g, res in enumerate(secagg.close_groups(gpu_ctx, full, RND)):
        assert res["sum"] == grads[16 * g:16 * g + 16].sum(axis=0).tolist(), g
    out = {1000, 1015, 1020, 1033, 1034}                                       # 2 + 1 + 2 + 0 across the groups
    part = []
    for r in rosters:
        inc, exc = [i for i in r if i not in out], [i for i in r if i in out]
        pairs = [(i, j) for i in inc for j in exc]
        keys = secagg.fr_ints(secagg.harness_keys(gpu_ctx, pairs)) if pairs else []
        part.append({"roster": r, "accepted": {i: masked[index[i]] for i in inc},
                     "revealed": [(i, j, k) for (i, j), k in zip(pairs, keys)]})
    for g, res in enumerate(secagg.close_groups(gpu_ctx, part, RND)):
        rows = [index[i] for i in part[g]["accepted"]]
        assert res["sum"] == grads[rows].sum(axis=0).tolist() and not res["out_of_range"], g
    assert part[0]["revealed"][0][2] == clients.shared_key(1001, 1000)         # the harness's key, from the CPU


def _arg_error(match, fn, *args, **kw):
    with pytest.raises(native.ZkflError, match=match) as e:
        fn(*args, **kw)
    assert e.value.code == -1, e.value


def test_argument_errors_name_the_index_and_leave_the_context_usable(gpu_ctx):
    ctx = gpu_ctx
    big = R.to_bytes(32, "little")
    k = [x.to_bytes(32, "little") for x in _keys(8, 3)]
    g2 = M.fr_bytes([[1, 2], [3, 4]])
    mask = ctx.secagg_mask
    _arg_error("key 1 is not < r", mask, [1, 2], [0, 1, 2], [2, 1], k[0] + big, RND, g2, 2)
    _arg_error("gradient value 2 is not < r", mask, [1, 2], [0, 1, 2], [2, 1], k[0] + k[1], RND, g2[:64] + big + g2[96:], 2)
    _arg_error("round 0 is not < r", mask, [1, 2], [0, 1, 2], [2, 1], k[0] + k[1], R, g2, 2)
    _arg_error("dim must be at least 1", mask, [1, 2], [0, 1, 2], [2, 1], k[0] + k[1], RND, b"", 0)
    _arg_error(r"peer_ptr\[2\] is below peer_ptr\[1\]", mask, [1, 2], [0, 2, 1], [2], k[0], RND, g2, 2)
    _arg_error(r"peer_ptr\[0\] must be 0", mask, [1, 2], [1, 1, 2], [2, 1], k[0] + k[1], RND, g2, 2)
    _arg_error(r"client 1: peer_ids\[1\] is the client's own id", mask, [1, 2], [0, 1, 2], [2, 2], k[0] + k[1], RND, g2, 2)
    _arg_error(r"client 0: peer_ids\[2\] repeats peer_ids\[0\]", mask, [1, 2], [0, 3, 3], [5, 6, 5], b"".join(k), RND, g2, 2)
    _arg_error(r"peer_ptr\[1\] = 4294967296 peers: must be < 2\^32", mask, [1], [0, 1 << 32], [2], k[0], RND, g2[:64], 2)
    agg = ctx.secagg_aggregate
    _arg_error("masked value 3 is not < r", agg, [0, 2], g2[:96] + big, [0, 1], [1], [9], k[0], RND, 2)
    _arg_error("pair key 0 is not < r", agg, [0, 2], g2, [0, 1], [1], [9], big, RND, 2)
    _arg_error("round 0 is not < r", agg, [0, 2], g2, [0, 1], [1], [9], k[0], R, 2)
    _arg_error("dim must be at least 1", agg, [0, 2], b"", [0, 1], [1], [9], k[0], RND, 0)
    _arg_error(r"pair 1: pair_in equals pair_out", agg, [0, 2], g2, [0, 2], [1, 9], [9, 9], k[0] + k[1], RND, 2)
    _arg_error(r"member_ptr\[2\] is below member_ptr\[1\]", agg, [0, 2, 1], g2[:64], [0, 0, 0], [], [], b"", RND, 2)
    _arg_error(r"pair_ptr\[2\] is below pair_ptr\[1\]", agg, [0, 1, 2], g2, [0, 1, 0], [], [], b"", RND, 2)
    _arg_error(r"pair_ptr\[1\] = 4294967296 pairs: must be < 2\^32", agg, [0, 2], g2, [0, 1 << 32], [1], [9], k[0], RND, 2)
    # nothing to do is valid
    assert mask([], [0], [], b"", RND, b"", 2).shape == (0, 2, 32)
    sums, sg, oor = agg([0], b"", [0], [], [], b"", RND, 2)
    assert sums.shape == (0, 2, 32) and sg.shape == (0, 2) and oor.shape == (0,)
    # and the context still works
    a = RAGGED
    got = secagg.mask_updates(ctx, a["ids"], a["peers"], a["keys"], RND, a["grads"])
    assert got.tobytes() == _model_bytes(a["ids"], a["peers"], a["keys"], RND, a["grads"])


def _aggregate_round(path, cwd):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT)
    return subprocess.run([sys.executable, "-m", "zkfl", "aggregate-round", str(path)], cwd=cwd, env=env,
                          capture_output=True, text=True, timeout=300)


def test_aggregate_round_command(tmp_path, two_groups):
    groups, want = two_groups
    man = {"round": RND, "dim": 3, "groups": []}
    for g, grp in enumerate(groups):
        cl = []
        for i in grp["roster"]:
            c = {"id": i, "accepted": i in grp["accepted"]}
            if c["accepted"]:
                c["public"] = f"g{g}/public_{i}.json"
                os.makedirs(tmp_path / f"g{g}", exist_ok=True)
                sig = [i, RND, 1, 2, 3, 4, 10 ** 8] + grp["accepted"][i]
                (tmp_path / c["public"]).write_text(json.dumps([str(x) for x in sig]))
            cl.append(c)
        man["groups"].append({"clients": cl, "revealed": [{"in": i, "out": j, "key": str(k)}
                                                           for i, j, k in grp["revealed"]]})
    (tmp_path / "round.json").write_text(json.dumps(man))
    out = _aggregate_round(tmp_path / "round.json", tmp_path)
    assert out.returncode == 0, out.stderr
    lines = [json.loads(x) for x in out.stdout.splitlines()]
    assert lines == [{"group": g, "clients": len(grp["accepted"]), "sum": want[g],
                      "mean": [x / len(grp["accepted"]) for x in want[g]]} for g, grp in enumerate(groups)]
    # a wrong key leaves a mask in group 0's sum: exit 1, no sum for it, group 1 unharmed
    man["groups"][0]["revealed"][3]["key"] = str((int(man["groups"][0]["revealed"][3]["key"]) + 1) % R)
    (tmp_path / "wrong_key.json").write_text(json.dumps(man))
    out = _aggregate_round(tmp_path / "wrong_key.json", tmp_path)
    assert out.returncode == 1, out.stderr
    lines = [json.loads(x) for x in out.stdout.splitlines()]
    assert lines[0] == {"group": 0, "clients": 4, "sum": None, "mean": None, "out_of_range": True}
    assert lines[1]["sum"] == want[1]
