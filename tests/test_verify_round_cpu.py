"""The combined round check's surface without a GPU: the header and the library carry the two
entry points and the report struct, their null-argument paths answer without a device,
`python -m zkfl verify-round --combined` rejects a bad manifest (exit 2) before it creates a
context, and the identity the GPU path rests on holds in the Python tower: the product of the
per-job check values raised to z_i equals the sums-first formula (one pair per job, three per key,
one final exponentiation)."""
import ctypes
import json
import os
import random
import re
import subprocess
import sys

from oracle import bn254 as bn
from oracle import pairing_tower as T
from zkfl import native

import verify_round_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(native.LIB_PATH)

NEW = ("zkfl_groth16_verify_round", "zkfl_debug_verify_round")


def test_header_declares_and_library_exports_the_round_functions():
    src = open(os.path.join(ROOT, "include", "zkfl.h")).read()
    declared = set(re.findall(r"\b(zkfl_[a-z0-9_]+)\s*\(", src))
    lib = ctypes.CDLL(native.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in native.SIGNATURES, name
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*zkfl_round_report\s*;", src)
    assert m, "zkfl_round_report"
    fields = re.findall(r"uint32_t\s+([a-z_]+)\s*;", m.group(1))
    assert tuple(fields) == ("keys", "screened", "combined", "passed", "fallback")
    assert tuple(fields) == native.ROUND_REPORT_FIELDS
    for rec in ("verify_round_screen", "verify_round_pair", "verify_round_reduce", "verify_round_final"):
        assert f'"{rec}"' in src, rec
    # the existing schedules keep their meaning
    assert native.VERIFY_SCHEDULES == {"auto": 0, "lanes": 1, "waves": 2}


def test_null_arguments_answer_without_a_device():
    L = native.lib()
    assert L.zkfl_groth16_verify_round(None, 0, None, None, None, None, None, None, None) == -1
    assert L.zkfl_groth16_verify_round(None, 1, None, None, None, None, None, None, None) == -1
    out = (ctypes.c_uint8 * 384)()
    assert L.zkfl_debug_verify_round(None, 0, None, None, None, None, None, 0, out, None) == -1
    assert L.zkfl_debug_verify_round(None, 1, None, None, None, None, None, 0, None, None) == -1
    assert bytes(out) == bytes(384)
    assert "verify_round" in L.zkfl_last_error().decode()


def _verify_round(path, cwd):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT)
    return subprocess.run([sys.executable, "-m", "zkfl", "verify-round", "--combined", str(path)], cwd=cwd, env=env,
                          capture_output=True, text=True, timeout=120)


def test_verify_round_combined_rejects_bad_manifests_before_any_device_use(tmp_path):
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


def test_product_of_powers_equals_sums_first_on_random_points():
    rng = random.Random(20261020)
    g1 = lambda: bn.mul(bn.G1_GEN, rng.randrange(1, bn.R))  # noqa: E731
    g2 = lambda: bn.mul(bn.G2_GEN, rng.randrange(1, bn.R))  # noqa: E731
    keys = [(g1(), g2(), g2(), g2()) for _ in range(2)]
    jobs = [(g1(), g2(), g1(), g1(), i % 2) for i in range(5)]
    jobs[3] = (None,) + jobs[3][1:]  # an infinite pi_a: its pair contributes 1
    zs = [1, (1 << 128) - 1, rng.randrange(1 << 128), 0, rng.randrange(1 << 128)]
    values = [M.check_value(A, B, X, C, keys[k]) for A, B, X, C, k in jobs]
    want = M.product_of_powers(values, zs)
    assert M.sums_first(jobs, keys, zs) == want
    assert T.gt_bytes(want) != M.GT_ONE  # random points: not a valid round
    # one job, z = 1: the check value itself
    assert M.sums_first(jobs[:1], keys, [1]) == values[0]
