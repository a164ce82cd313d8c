"""The narrowed round check's surface without a GPU: the header and the library carry the two
entry points, the report struct and the two policy constants, their null-argument paths answer
without a device, the model's grouping rule (tests/narrow_model.py) gives the hand-written
groups, and `python -m zkfl verify-round --narrow` rejects a bad manifest (exit 2) before it
creates a context."""
import ctypes
import json
import os
import re
import subprocess
import sys

from zkfl import native

import narrow_model as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(native.LIB_PATH)

NEW = ("zkfl_groth16_verify_round_narrow", "zkfl_debug_verify_round_groups")


def test_header_declares_and_library_exports_the_narrow_functions():
    src = open(os.path.join(ROOT, "include", "zkfl.h")).read()
    declared = set(re.findall(r"\b(zkfl_[a-z0-9_]+)\s*\(", src))
    lib = ctypes.CDLL(native.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in native.SIGNATURES, name
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*zkfl_narrow_report\s*;", src)
    assert m, "zkfl_narrow_report"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [f.strip() for decl in re.findall(r"uint32_t\s+([a-z_,\s]+);", body) for f in decl.split(",")]
    assert tuple(fields) == ("keys", "screened", "combined", "passed", "groups", "bad_groups", "fallback")
    assert tuple(fields) == native.NARROW_REPORT_FIELDS
    assert native.NARROW_REPORT_FIELDS[:4] == native.ROUND_REPORT_FIELDS[:4]
    assert '"verify_round_groups"' in src
    for name, value in (("ZKFL_ROUND_GROUP", native.ROUND_GROUP), ("ZKFL_ROUND_NARROW_MIN", native.ROUND_NARROW_MIN)):
        d = re.search(rf"#define\s+{name}\s+(\d+)", src)
        assert d and int(d.group(1)) == value, name
    assert N.ROUND_GROUP == native.ROUND_GROUP


def test_null_arguments_answer_without_a_device():
    L = native.lib()
    assert L.zkfl_groth16_verify_round_narrow(None, 0, None, None, None, None, None, 0, None, None) == -1
    assert L.zkfl_groth16_verify_round_narrow(None, 1, None, None, None, None, None, 4, None, None) == -1
    assert "verify_round_narrow" in L.zkfl_last_error().decode()
    ng = ctypes.c_uint32(77)
    out = (ctypes.c_uint8 * 384)()
    assert L.zkfl_debug_verify_round_groups(None, 0, None, None, None, None, None, 0, 0, None, out, 1,
                                            ctypes.byref(ng), None) == -1
    assert L.zkfl_debug_verify_round_groups(None, 1, None, None, None, None, None, 0, 1, None, None, 0, None,
                                            None) == -1
    assert "verify_round_groups" in L.zkfl_last_error().decode()
    assert ng.value == 77 and bytes(out) == bytes(384)


def test_grouping_on_hand_written_cases():
    # a key border inside a group: keys a b a b a b a -> order a0 a2 a4 a6 | b1 b3 b5, groups of 3
    g, ng = N.grouping(list("abababa"), 0, 3)
    assert (g, ng) == ([0, 1, 0, 1, 0, 2, 1], 3)  # group 1 holds a6, b1, b3; group 2 is short (b5)
    # keys in order of first appearance, not of their names
    g, ng = N.grouping(list("bab"), 0, 2)
    assert (g, ng) == ([0, 1, 0], 2)
    # a pass border: 7 jobs of one key, passes of 5, groups of 2 -> 2 2 1 | 2
    g, ng = N.grouping(["k"] * 7, 5, 2)
    assert (g, ng) == ([0, 0, 1, 1, 2, 3, 3], 4)
    # ... and with two keys the border cuts the sorted order, not the job order
    g, ng = N.grouping(list("abababa"), 5, 2)  # order a0 a2 a4 a6 b1 | b3 b5
    assert (g, ng) == ([0, 2, 0, 3, 1, 3, 1], 4)
    # a short last group; group = 1; the production size
    assert N.grouping(["k"] * 5, 0, 4) == ([0, 0, 0, 0, 1], 2)
    assert N.grouping(list("abab"), 0, 1) == ([0, 2, 1, 3], 4)
    assert N.grouping(["k"] * 70, 0, 0) == ([0] * 64 + [1] * 6, 2)
    assert N.grouping(["k"] * 3, 0, 0) == ([0, 0, 0], 1)
    assert N.grouping([], 0, 0) == ([], 0)
    # the report: the bad jobs' groups, and their unscreened jobs
    rep = N.expected_report(["k"] * 8, [False, True] + [False] * 6, [True, False, False] + [True] * 5, 0, 2)
    assert rep == {"screened": 1, "combined": 7, "passed": 0, "groups": 4, "bad_groups": 1, "fallback": 2}
    rep = N.expected_report(["k"] * 4, [False, True, False, False], [True, False, True, True], 0, 2)
    assert rep == {"screened": 1, "combined": 3, "passed": 1, "groups": 2, "bad_groups": 0, "fallback": 0}


def _verify_round(path, cwd):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT)
    return subprocess.run([sys.executable, "-m", "zkfl", "verify-round", "--narrow", str(path)], cwd=cwd, env=env,
                          capture_output=True, text=True, timeout=120)


def test_verify_round_narrow_rejects_bad_manifests_before_any_device_use(tmp_path):
    for name in ("vkey.json", "public.json", "proof.json"):
        (tmp_path / name).write_text("{}")
    good = {"vkey": "vkey.json", "public": "public.json", "proof": "proof.json"}
    cases = {
        "not_a_list.json": {"jobs": [good]},
        "missing_proof.json": [good, {"vkey": "vkey.json", "public": "public.json"}],
        "missing_file.json": [good, dict(good, proof="nowhere.json")],
    }
    for name, manifest in cases.items():
        (tmp_path / name).write_text(json.dumps(manifest))
        out = _verify_round(tmp_path / name, tmp_path)
        # exit 2 comes from the manifest check; a context would fail otherwise (no GPU: exit 1)
        assert out.returncode == 2, (name, out.stdout, out.stderr)
        assert out.stdout == "", name
    out = _verify_round(tmp_path / "absent.json", tmp_path)
    assert out.returncode == 2
