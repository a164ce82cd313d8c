"""bench.py's reproducible inputs and its --dump-outputs writer (CPU): the blinding factors of the
timed proofs come from a seeded generator, and a dumped proof round-trips through float32 exactly."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_draw_rs_seeded_and_in_range():
    bench = _bench()
    from zkfl.field import R
    a, b = bench.draw_rs(5), bench.draw_rs(5)
    assert a == b and len(a) == 5 * 64
    assert bench.draw_rs(3) == a[:3 * 64]                      # a longer run extends a shorter one
    assert bench.draw_rs(5, bench.RS_SEED + 1) != a            # another rank's factors differ
    vals = [int.from_bytes(a[32 * i:32 * i + 32], "little") for i in range(10)]
    assert all(0 <= v < R for v in vals) and len(set(vals)) == 10


def test_dump_outputs_roundtrip(tmp_path):
    import numpy as np
    bench = _bench()
    proofs = [bytes((7 * i + j) % 256 for j in range(256)) for i in range(3)]
    bench.dump_outputs(str(tmp_path / "out"), "proofs", proofs)
    arr = np.load(tmp_path / "out" / "proofs.npy")
    assert arr.dtype == np.float32 and arr.shape == (3, 256)
    assert [bytes(row.astype(np.uint8)) for row in arr] == proofs
