"""Secure aggregation without a GPU: the model (tests/secagg_model.py) against zkfl/clients.py, the
cancellation identity and what an uncorrected sum looks like, the library's surface, the key checks
of zkfl/secagg.py::close_groups and the exit codes of `python -m zkfl aggregate-round` on manifests
that must be refused before a context exists."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from zkfl import clients, native, secagg
from zkfl.field import R

import secagg_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(native.LIB_PATH)

IDS = [1, 2, 3, 5, 9]
RND = 4
GRADS = {1: [5, -7], 2: [0, 11], 3: [-1, 1 << 40], 5: [123456, -(1 << 33)], 9: [7, 7]}
OUT = {3, 9}


@pytest.fixture(scope="module")
def group():
    """The clients' inputs from zkfl/clients.py and the model's masked updates (dim 2)."""
    inputs = {i: clients.secagg_input(i, [p for p in IDS if p != i], GRADS[i], RND, 10 ** 8, 1, 2) for i in IDS}
    keys = {(i, p): int(k) for i in IDS
            for p, k in zip([p for p in IDS if p != i], inputs[i]["shared_keys"])}
    masked = {i: M.mask(i, [p for p in IDS if p != i], [keys[i, p] for p in IDS if p != i], RND, GRADS[i])
              for i in IDS}
    return inputs, keys, masked


def test_model_equals_clients_secagg_input(group):
    inputs, keys, masked = group
    for i in IDS:
        assert [str(x) for x in masked[i]] == inputs[i]["masked_update"], i
    assert keys[1, 9] == keys[9, 1] == clients.shared_key(1, 9)


def test_full_group_sum_is_the_sum_of_the_gradients(group):
    _, _, masked = group
    total = M.aggregate([masked[i] for i in IDS], [], RND)
    want = [sum(GRADS[i][k] for i in IDS) for k in range(2)]
    assert [M.signed(v) for v in total] == want
    assert M.decode(total) == (want, False)


def test_excluded_clients_leave_masks_that_the_revealed_keys_take_out(group):
    _, keys, masked = group
    inc = [i for i in IDS if i not in OUT]
    pairs = [(i, j, keys[i, j]) for i in inc for j in sorted(OUT)]
    want = [sum(GRADS[i][k] for i in inc) for k in range(2)]
    assert M.decode(M.aggregate([masked[i] for i in inc], pairs, RND)) == (want, False)
    raw = M.aggregate([masked[i] for i in inc], [], RND)
    assert all(abs(M.signed(v)).bit_length() > 200 for v in raw)     # field-sized: the masks are still in it
    assert M.decode(raw) == ([0, 0], True)
    assert M.decode([M.INT64_MAX, (M.INT64_MIN) % R]) == ([M.INT64_MAX, M.INT64_MIN], False)
    assert M.decode([M.INT64_MAX + 1])[1] and M.decode([(M.INT64_MIN - 1) % R])[1]


def test_packing_of_signed_integers():
    vals = np.array([[0, 1, -1], [M.INT64_MAX, M.INT64_MIN + 1, -(1 << 32)]], dtype=np.int64)
    got = secagg.fr_bytes(vals)
    assert got.shape == (2, 3, 32)
    assert secagg.fr_ints(got) == [[int(v) % R for v in row] for row in vals]
    assert secagg.fr_bytes([[R - 1, 5]]).tobytes() == M.fr_bytes([[R - 1, 5]])
    assert secagg.signed(R - 7) == -7 and secagg.signed(7) == 7


def test_close_groups_refuses_missing_duplicate_and_superfluous_keys(group):
    _, keys, masked = group
    inc = [i for i in IDS if i not in OUT]
    pairs = [(i, j, keys[i, j]) for i in inc for j in sorted(OUT)]
    grp = {"roster": IDS, "accepted": {i: masked[i] for i in inc}, "revealed": pairs}
    secagg.check_group(0, grp["roster"], list(grp["accepted"]), grp["revealed"])      # the good one passes
    # ctx None: the refusal must come before any use of the context
    with pytest.raises(ValueError, match=r"group 0: no revealed key for the pair \(5, 9\)"):
        secagg.close_groups(None, [dict(grp, revealed=pairs[:-1])], RND)
    with pytest.raises(ValueError, match=r"revealed key 6 names the pair \(1, 3\) a second time"):
        secagg.close_groups(None, [dict(grp, revealed=pairs + [pairs[0]])], RND)
    with pytest.raises(ValueError, match=r"revealed key 6 names the pair \(1, 2\), which is not"):
        secagg.close_groups(None, [dict(grp, revealed=pairs + [(1, 2, keys[1, 2])])], RND)
    with pytest.raises(ValueError, match=r"names the pair \(3, 1\), which is not"):            # the wrong way round
        secagg.close_groups(None, [dict(grp, revealed=[(3, 1, keys[1, 3])] + pairs[1:])], RND)
    with pytest.raises(ValueError, match="group 1: accepted client 4 is not in the roster"):
        secagg.close_groups(None, [grp, {"roster": [1, 2], "accepted": {4: [0, 0]}, "revealed": []}], RND)
    with pytest.raises(ValueError, match="no accepted client"):
        secagg.close_groups(None, [{"roster": [1, 2], "accepted": {}, "revealed": []}], RND)


def test_header_declares_and_library_exports_the_secagg_functions():
    src = open(os.path.join(ROOT, "include", "zkfl.h")).read()
    declared = set(re.findall(r"\b(zkfl_[a-z0-9_]+)\s*\(", src))
    lib = ctypes.CDLL(native.LIB_PATH)
    for name in ("zkfl_secagg_mask", "zkfl_secagg_aggregate"):
        assert name in declared and hasattr(lib, name) and name in native.SIGNATURES, name
    for rec in ("secagg_terms", "secagg_fold"):
        assert f'"{rec}"' in src, rec
    L = native.lib()
    assert L.zkfl_secagg_mask(None, 0, 1, None, None, None, None, None, None, None, 0) == -1
    assert "secagg_mask" in L.zkfl_last_error().decode()
    assert L.zkfl_secagg_aggregate(None, 0, 1, None, None, None, None, None, None, None, None, None, None, 0) == -1
    assert "secagg_aggregate" in L.zkfl_last_error().decode()


def _aggregate_round(path, cwd):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT)
    return subprocess.run([sys.executable, "-m", "zkfl", "aggregate-round", str(path)], cwd=cwd, env=env,
                          capture_output=True, text=True, timeout=120)


def test_aggregate_round_rejects_unusable_manifests_before_any_device_use(tmp_path):
    def public(cid, rnd=RND):
        return [str(x) for x in [cid, rnd, 0, 0, 0, 0, 10 ** 8, 11, 22]]

    for cid in (1, 2):
        (tmp_path / f"pub{cid}.json").write_text(json.dumps(public(cid)))
    (tmp_path / "pub2_round5.json").write_text(json.dumps(public(2, 5)))
    cl = [{"id": 1, "accepted": True, "public": "pub1.json"}, {"id": 2, "accepted": True, "public": "pub2.json"},
          {"id": "3", "accepted": False}]
    rev = [{"in": 1, "out": 3, "key": "77"}, {"in": 2, "out": 3, "key": "78"}]

    def man(clients_=cl, revealed=rev, **top):
        return dict({"round": RND, "dim": 2, "groups": [{"clients": clients_, "revealed": revealed}]}, **top)

    cases = {
        "a_list.json": [man()],
        "no_dim.json": {"round": RND, "groups": man()["groups"]},
        "no_revealed.json": {"round": RND, "dim": 2, "groups": [{"clients": cl}]},
        "no_public.json": man([cl[0], {"id": 2, "accepted": True}, cl[2]]),
        "missing_file.json": man([cl[0], dict(cl[1], public="nowhere.json"), cl[2]]),
        "other_client.json": man([cl[0], dict(cl[1], public="pub1.json"), cl[2]]),
        "other_round.json": man([cl[0], dict(cl[1], public="pub2_round5.json"), cl[2]]),
        "other_dim.json": man(dim=3),
        "missing_key.json": man(revealed=rev[:1]),
        "unneeded_key.json": man(revealed=rev + [{"in": 1, "out": 2, "key": "79"}]),
        "repeated_key.json": man(revealed=rev + [rev[0]]),
    }
    for name, manifest in cases.items():
        (tmp_path / name).write_text(json.dumps(manifest))
        out = _aggregate_round(tmp_path / name, tmp_path)
        # exit 2 comes from the manifest check; a context would fail otherwise (no GPU: exit 1)
        assert out.returncode == 2, (name, out.stdout, out.stderr)
        assert out.stdout == "" and "[ERROR] zkfl" in out.stderr, name
    assert _aggregate_round(tmp_path / "absent.json", tmp_path).returncode == 2
