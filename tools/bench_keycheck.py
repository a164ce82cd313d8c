"""Time `zkey check` against the only other way to test a key's sections 3, 5, 6, 7: running
`groth16 setup` (zkfl/zkey.py setup_from_ptau) again and comparing bytes.

    python tools/bench_keycheck.py [circuit params..]    default: sgd_verified 8 4 3

One process, one context: a dev ptau at the circuit's power + 1 is made on the GPU, the key is set up
from it and contributed to once, then after one warm-up call each the wall time of zkfl_zkey_check
(its four profiler stages beside it) and of setup_from_ptau, median [min, max] of 5.  Prints one JSON
line (DESIGN.md §16 quotes it).
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "verifiable-federated-training-with-zero-knowledge-proofs-zk-fl-_amd")]

from zkfl import circuits, native, ptau, zkey  # noqa: E402

STAGES = ("keycheck_points", "keycheck_rows", "keycheck_msm", "keycheck_pairing")


def _note(msg):
    print(f"[bench_keycheck] {msg}", file=sys.stderr, flush=True)


def _stats(xs):
    return [round(statistics.median(xs), 3), round(min(xs), 3), round(max(xs), 3)]


def main(argv):
    name, params = (argv[0], tuple(int(x) for x in argv[1:])) if argv else ("sgd_verified", (8, 4, 3))
    b = circuits.build(name, *params)
    r1cs = b.r1cs_bytes()
    n = zkey.domain_size_for(b)
    power = n.bit_length() - 1
    os.environ["ZKFL_DETERMINISTIC_SETUP"] = "1"
    out = {"circuit": [name, *params], "wires": b.n_wires, "constraints": b.n_constraints, "domain": n,
           "ptau_power": power + 1}
    with native.Context(0) as ctx:
        t0 = time.perf_counter()
        pt = ptau.prepare_phase2(ptau.contribute(ptau.new(power + 1), ctx, 0x2468ACE13579, 0x1111, 0x2222), ctx)
        out["ptau_s"] = round(time.perf_counter() - t0, 2)
        _note(f"ptau of power {power + 1} made in {out['ptau_s']} s")
        zk = zkey.zkey_contribute(zkey.setup_from_ptau(b, pt, ctx), ctx, 0x3333)
        out["zkey_bytes"] = len(zk)
        _note(f"key of {len(zk)} bytes set up")
        t0 = time.perf_counter()
        blocks = zkey.ptau_blocks(b, pt)
        out["block_selection_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
        with native.R1cs(ctx, r1cs) as cs:
            assert cs.check_key(zk, blocks).ok          # warm-up
            ctx.set_profiling(True)
            wall, stages = [], {s: [] for s in STAGES}
            for _ in range(5):
                ctx.profile_reset()
                t0 = time.perf_counter()
                rep = cs.check_key(zk, blocks)
                wall.append(1e3 * (time.perf_counter() - t0))
                assert rep.ok
                for s in STAGES:
                    stages[s].append(ctx.profile(s)[0])
            ctx.profile_reset()
            ctx.set_profiling(False)
        out["check_ms"] = _stats(wall)
        _note(f"check_ms {out['check_ms']}")
        out["stages_ms"] = {s: _stats(v) for s, v in stages.items()}
        zkey.setup_from_ptau(b, pt, ctx)                # warm-up
        wall = []
        for _ in range(5):
            t0 = time.perf_counter()
            zkey.setup_from_ptau(b, pt, ctx)
            wall.append(1e3 * (time.perf_counter() - t0))
            _note(f"setup_from_ptau {wall[-1]:.0f} ms")
        out["setup_from_ptau_ms"] = _stats(wall)
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1:])
