"""Multi-key verification surface without a GPU: the header and the library carry the new entry
points, their null-argument paths answer without a device, and `python -m zkfl verify-round`
rejects a bad manifest (exit 2) before it creates a context."""
import ctypes
import json
import os
import re
import subprocess
import sys

from zkfl import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(native.LIB_PATH)

NEW = ("zkfl_vkey_load", "zkfl_vkey_info", "zkfl_vkey_free", "zkfl_groth16_verify_multi",
       "zkfl_debug_wave_pairing")


def test_header_declares_and_library_exports_the_new_functions():
    src = open(os.path.join(ROOT, "include", "zkfl.h")).read()
    declared = set(re.findall(r"\b(zkfl_[a-z0-9_]+)\s*\(", src))
    lib = ctypes.CDLL(native.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in native.SIGNATURES, name
    for macro, value in (("ZKFL_VERIFY_AUTO", 0), ("ZKFL_VERIFY_LANES", 1), ("ZKFL_VERIFY_WAVES", 2)):
        assert re.search(rf"#define\s+{macro}\s+{value}\b", src), macro
    assert native.VERIFY_SCHEDULES == {"auto": 0, "lanes": 1, "waves": 2}
    assert re.search(r"#define\s+ZKFL_VERIFY_AUTO_WAVES_MAX\s+\d+", src)
    assert re.search(r"#define\s+ZKFL_VERIFY_WAVE_MAX_PUBLIC\s+\d+", src)


def test_null_arguments_answer_without_a_device():
    L = native.lib()
    n = ctypes.c_uint32(7)
    assert L.zkfl_vkey_info(None, ctypes.byref(n)) == -1
    assert n.value == 7
    assert L.zkfl_vkey_free(None) == -1
    assert L.zkfl_groth16_verify_multi(None, 0, None, None, None, None, None, 0) == -1
    assert L.zkfl_vkey_load(None, None, 0, None) == -1
    assert L.zkfl_debug_wave_pairing(None, 0, None, None, 1, None) == -1


def _verify_round(path, cwd):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT)
    return subprocess.run([sys.executable, "-m", "zkfl", "verify-round", str(path)], cwd=cwd, env=env,
                          capture_output=True, text=True, timeout=120)


def test_verify_round_rejects_bad_manifests_before_any_device_use(tmp_path):
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
