#!/usr/bin/env python3
"""Groth16 verification on the GPU: latency (batch 1) and throughput (batched, one lane per proof).

Circuit: sgd_verified(8,4,3,1000) (6 public signals), dev ceremony, one proof replicated.
Prints one JSON line per batch size.  Not part of the bench.py contract (verification is a
correctness gate in SURVEY.md §8 a9, not the metric).

    bench_verify.py [sizes..]            one key, zkfl_groth16_verify_batch
    bench_verify.py --multi [sizes..]    two resident keys, zkfl_groth16_verify_multi: one line per
                                         (schedule, n), lanes and waves in the same process
    bench_verify.py --round [sizes..]    the --multi setup; per n one line each for lanes, waves and the
                                         combined call (zkfl_groth16_verify_round) in the same process,
                                         the combined call's per-stage records, and one round with a
                                         single invalid proof (the fallback's cost)
    bench_verify.py --narrow [--group G] [sizes..]   the --round setup; per (n, invalid proofs) the
                                         combined call against zkfl_groth16_verify_round_narrow
                                         (groups of G, default 64), alternating in the same process
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "verifiable-federated-training-with-zero-knowledge-proofs-zk-fl-_amd"), ROOT]

from zkfl import circuits, clients, groth16, native, wprog  # noqa: E402
from zkfl import zkey  # noqa: E402


def _two_keys(ctx):
    """Two resident keys with one valid proof each: sgd_verified(8,4,3) and secure_masked_update(4,7)
    (bench.py config 5's pair) -> [(VerifyingKey, public bytes, proof bytes)]."""
    tr, sa, _ = clients.federated_round(8, rnd=1)[0]
    made = []
    for i, (b, inp) in enumerate(((circuits.build("sgd_verified", 8, 4, 3, 1000), tr),
                                  (circuits.build("secure_masked_update", 4, 7), sa))):
        zk = zkey.groth16_setup(b, ctx, zkey.Toxic(tau=0xC5 + i, alpha=3, beta=5, gamma=7, delta=11 + i))
        key = native.ProvingKey(ctx, zk)
        wp = native.WitnessProgram(ctx, wprog.compile_program(b))
        proof, pub = key.prove(wp.compute([wprog.input_bytes(b, inp)])[0])
        wp.close()
        key.close()
        vk = native.VerifyingKey(ctx, groth16.vk_bytes(groth16.export_verification_key(zk, alphabeta=False)))
        made.append((vk, groth16.public_bytes(pub), proof))
    return made


def _timed(label, n, made, call, want, repeats, **extra):
    """One JSON line: median, min and max wall time of `repeats` calls after one warm-up call whose
    verdicts are checked."""
    import statistics
    assert call() == want, label  # warm-up, and the verdicts
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"schedule": label, "n": n, "median_ms": round(statistics.median(ts), 3),
                      "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "repeats": repeats,
                      "npub": [made[0][0].n_public, made[1][0].n_public], **extra,
                      "build": native.build_id()}), flush=True)


def multi(sizes, repeats=10):
    """--multi: a round's proofs against the two keys, interleaved as a round interleaves them
    (training, secure aggregation, training, ...).  One JSON line per (schedule, n): median, min and
    max wall time of `repeats` verify_multi calls after one warm-up call, same process, same jobs."""
    ctx = native.Context(0)
    made = _two_keys(ctx)
    for n in sizes:
        jobs = [made[i % 2] for i in range(n)]
        for sched in ("lanes", "waves"):
            _timed(sched, n, made, lambda: ctx.verify_multi(jobs, sched), [True] * n, repeats)
    # where the wave path's time goes: per-kernel event times of one proof and of a round of 16
    for n in (1, 16):
        ctx.set_profiling(True)
        ctx.profile_reset()
        ctx.verify_multi([made[i % 2] for i in range(n)], "waves")
        prof = {k: round(ctx.profile(k)[0], 3) for k in ("verify_wave_g2", "verify_wave_inputs", "verify_wave_pair")}
        ctx.set_profiling(False)
        print(json.dumps({"profile_ms": prof, "n": n}), flush=True)
    ctx.close()


ROUND_RECORDS = ("verify_round_screen", "verify_round_pair", "verify_round_reduce", "verify_round_final")


def round_(sizes, repeats=10):
    """--round: --multi's jobs under lanes, waves and the combined call, same process; then the
    combined call's per-stage event times, and the round with its last proof made invalid (pi_c + G:
    it passes the screening, so the combination fails and every job is verified again one by one)."""
    ctx = native.Context(0)
    made = _two_keys(ctx)
    vk, pub, proof = made[1]
    c = int.from_bytes(proof[192:224], "little"), int.from_bytes(proof[224:256], "little")
    from oracle import bn254 as bn
    bad_c = bn.add(c, bn.G1_GEN)
    bad = (vk, pub, proof[:192] + bad_c[0].to_bytes(32, "little") + bad_c[1].to_bytes(32, "little"))
    for n in sizes:
        jobs = [made[i % 2] for i in range(n)]
        for sched in ("lanes", "waves"):
            _timed(sched, n, made, lambda: ctx.verify_multi(jobs, sched), [True] * n, repeats)
        _timed("combined", n, made, lambda: ctx.verify_round(jobs)[0], [True] * n, repeats)
        ctx.set_profiling(True)
        ctx.profile_reset()
        _, rep = ctx.verify_round(jobs)
        prof = {k: round(ctx.profile(k)[0], 3) for k in ROUND_RECORDS}
        ctx.set_profiling(False)
        print(json.dumps({"profile_ms": prof, "n": n, "report": rep}), flush=True)
        one_bad = jobs[:-1] + [bad]
        _, rep = ctx.verify_round(one_bad)
        _timed("combined, one invalid proof", n, made, lambda: ctx.verify_round(one_bad)[0],
               [True] * (n - 1) + [False], repeats, report=rep)
    ctx.close()


NARROW_RECORDS = ROUND_RECORDS + ("verify_round_groups", "verify_wave_g2", "verify_wave_inputs", "verify_wave_pair")


def _plus_g(job):
    """The job with pi_c + G: it passes the screening and fails its check."""
    from oracle import bn254 as bn
    vk, pub, proof = job
    c = bn.add((int.from_bytes(proof[192:224], "little"), int.from_bytes(proof[224:256], "little")), bn.G1_GEN)
    return vk, pub, proof[:192] + c[0].to_bytes(32, "little") + c[1].to_bytes(32, "little")


def narrow(sizes, group=64, repeats=10):
    """--narrow: --round's jobs with b invalid proofs (pi_c + G) in b distinct groups, b in 0, 1, 8
    and one per group.  Per (n, b) the existing combined call and the narrow call (groups of
    `group`) alternate in the same process, one warm-up call each whose verdicts are checked, then
    `repeats` timed calls each: one JSON line per route, then the narrow report and both routes'
    per-stage event times."""
    import statistics
    ctx = native.Context(0)
    made = _two_keys(ctx)
    bad = [_plus_g(j) for j in made]
    for n in sizes:
        n0 = (n + 1) // 2  # the call orders the jobs by key: position p holds job 2p, n0 + p job 2p + 1
        firsts = [off + g for off in range(0, n, 4096) for g in range(0, min(4096, n - off), group)]
        for b in dict.fromkeys((0, 1, 8, len(firsts))):
            if b > len(firsts):
                continue
            jobs = [made[i % 2] for i in range(n)]
            want = [True] * n
            for k in range(b):
                p = firsts[k * len(firsts) // b]
                i = 2 * p if p < n0 else 2 * (p - n0) + 1
                jobs[i], want[i] = bad[i % 2], False
            routes = {"verify_round": lambda: ctx.verify_round(jobs),
                      "verify_round_narrow": lambda: ctx.verify_round_narrow(jobs, None, group)}
            reports, ts = {}, {r: [] for r in routes}
            for r, call in routes.items():  # warm-up, and the verdicts
                got, reports[r] = call()
                assert got == want, (r, n, b)
            for _ in range(repeats):
                for r, call in routes.items():
                    t0 = time.perf_counter()
                    call()
                    ts[r].append((time.perf_counter() - t0) * 1e3)
            for r in routes:
                print(json.dumps({"route": r, "n": n, "bad": b, "group": group,
                                  "median_ms": round(statistics.median(ts[r]), 3), "min_ms": round(min(ts[r]), 3),
                                  "max_ms": round(max(ts[r]), 3), "repeats": repeats, "report": reports[r],
                                  "build": native.build_id()}), flush=True)
            for r, call in routes.items():
                ctx.set_profiling(True)
                ctx.profile_reset()
                call()
                prof = {k: round(ctx.profile(k)[0], 3) for k in NARROW_RECORDS}
                ctx.set_profiling(False)
                print(json.dumps({"profile_ms": prof, "route": r, "n": n, "bad": b}), flush=True)
    ctx.close()


def main():
    if "--narrow" in sys.argv[1:]:
        args = [x for x in sys.argv[1:] if x != "--narrow"]
        group = 64
        if "--group" in args:
            at = args.index("--group")
            group = int(args[at + 1])
            del args[at:at + 2]
        return narrow([int(x) for x in args] or [256, 1024, 4096, 8192], group)
    if "--round" in sys.argv[1:]:
        return round_([int(x) for x in sys.argv[1:] if x != "--round"] or [16, 256, 1024, 4096])
    if "--multi" in sys.argv[1:]:
        return multi([int(x) for x in sys.argv[1:] if x != "--multi"] or [1, 16, 64, 256, 1024, 4096])
    sizes = [int(x) for x in (sys.argv[1:] or ["1", "64", "1024", "8192"])]
    b = circuits.build("sgd_verified", 8, 4, 3, 1000)
    inp, _ = clients.Client(1, 8, 4, 3, clients.JsLcg(12345)).training_input(8, 1000, 100000000)
    ctx = native.Context(0)
    zk = zkey.groth16_setup(b, ctx, zkey.Toxic(tau=77, alpha=1, beta=2, gamma=3, delta=4))
    key = native.ProvingKey(ctx, zk)
    wp = native.WitnessProgram(ctx, wprog.compile_program(b))
    proof, pub = key.prove(wp.compute([wprog.input_bytes(b, inp)])[0])
    vk = groth16.vk_bytes(groth16.export_verification_key(zk, alphabeta=False))
    pubb = groth16.public_bytes(pub)
    assert ctx.verify(vk, pubb, proof)  # also prepares and caches the key
    for n in sizes:
        reps = max(1, min(20, 2048 // n))
        t0 = time.perf_counter()
        for _ in range(reps):
            res = ctx.verify_batch(vk, pubb * n, proof * n, len(pub))
        dt = (time.perf_counter() - t0) / reps
        assert all(res)
        print(json.dumps({"batch": n, "ms_per_batch": round(dt * 1e3, 3), "verifications_per_s": round(n / dt, 1),
                          "npub": len(pub)}), flush=True)
    key.close()
    ctx.close()


if __name__ == "__main__":
    main()
