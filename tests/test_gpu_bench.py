"""A plain bench.py run and its --dump-outputs — MI355X (-m gpu).

`bench.py --gpus 1 --steps K --warmup W` (no --full) sets up, warms up, times K steps and prints
the line: the headline fields are there, the legs of --full are null.  --dump-outputs DIR writes
the last timed step's proofs; two runs with the same arguments write the same bytes (seeded r, s,
seeded clients, fixed dev ceremony), and since a plain run verifies nothing itself, the dumped
proofs are verified here by the GPU batch verifier against a key and public signals rebuilt from the
same constants.  Run on the small training circuit C2 = sgd_verified(8, 4, 3, 1000).
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP, SLOTS, CLIENTS = 3, 1, 4, 4


def _plain_run(out_dir):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
           "--circuit", "C2", "--slots", str(SLOTS), "--clients", str(CLIENTS), "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    log = p.stdout + "\n" + p.stderr
    assert p.returncode == 0, log[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, log[-4000:]
    return json.loads(lines[0]), log


def test_plain_run_line_and_reproducible_dump(tmp_path, gpu_ctx):
    import numpy as np
    from zkfl import circuits, clients, groth16, native, wprog, zkey
    rep, log = _plain_run(tmp_path / "a")
    rep2, _ = _plain_run(tmp_path / "b")
    # the headline fields, with --steps really the number of timed steps
    assert rep["metric"].startswith("Groth16 proofs/sec") and rep["unit"] == "proofs/s"
    assert rep["higher_is_better"] is True and rep["dtype"] == "u32" and rep["full"] is False
    assert rep["steps"] == STEPS and rep["warmup"] == WARMUP and rep["proofs_timed"] == STEPS * SLOTS
    assert f"[bench r0] {STEPS * SLOTS} proofs in" in log
    assert rep["ms_per_step"] > 0
    assert abs(rep["value"] - SLOTS / (rep["ms_per_step"] / 1e3)) <= 1e-3 * rep["value"]
    # nothing but the timed path ran
    for leg in ("roofline", "stage_ms_isolated_per_proof", "verified", "oracle_match", "end_to_end", "c5", "c5_weak",
                "extra_circuit", "latency_single_proof", "dataset_commit", "cli_prove", "cpu_baseline"):
        assert rep[leg] is None, leg
    for tag in ("config 5", "one proof alone", "end to end", "dataset commitment", "cli prove"):
        assert tag not in log, tag
    # the dump: the last step's proofs, byte for byte the same in both runs
    assert sorted(os.listdir(tmp_path / "a")) == ["proofs.npy"]
    a, b_ = np.load(tmp_path / "a" / "proofs.npy"), np.load(tmp_path / "b" / "proofs.npy")
    assert a.dtype == np.float32 and a.shape == (SLOTS, 256)
    assert np.array_equal(a, b_) and rep2["proofs_timed"] == rep["proofs_timed"]
    assert np.array_equal(a, np.round(a)) and a.min() >= 0 and a.max() <= 255
    proofs = [bytes(row.astype(np.uint8)) for row in a]
    assert len(set(proofs)) == SLOTS                      # distinct clients and distinct (r, s)
    # ... and they are valid proofs of bench.py's clients under bench.py's dev key
    batch, dim, depth, precision = 8, 4, 3, 1000
    b = circuits.build("sgd_verified", batch, dim, depth, precision)
    zk = zkey.groth16_setup(b, gpu_ctx, zkey.Toxic(tau=0x5EED, alpha=0xA1, beta=0xB2, gamma=0xC3, delta=0xD4))
    wp = native.WitnessProgram(gpu_ctx, wprog.compile_program(b))
    inputs = [wprog.input_bytes(b, clients.Client(c + 1, batch, dim, depth, clients.JsLcg(12345 + c))
                                .training_input(batch, precision, 100000000)[0]) for c in range(CLIENTS)]
    wts = wp.compute(inputs)
    wp.close()
    vk = groth16.export_verification_key(zk, alphabeta=False)
    npub = int(vk["nPublic"])
    pubs = [w[76 + 32:76 + 32 * (1 + npub)] for w in wts]      # wtns v2: header 76 B, wire 0 = 1
    # timed proof i uses client i mod CLIENTS; the last step starts at (STEPS - 1) * SLOTS
    first = (STEPS - 1) * SLOTS
    vk = groth16.vk_bytes(vk)
    ok = gpu_ctx.verify_batch(vk, b"".join(pubs[(first + j) % CLIENTS] for j in range(SLOTS)), b"".join(proofs), npub)
    assert ok == [True] * SLOTS
