"""Time the fused mask engine (zkfl_secagg_mask) against the route to the same bytes that the
library offered before it: Poseidon rows built on the host, zkfl_poseidon_batch(arity 5), signed
sums on the host.

    python tools/bench_secagg.py [--groups 128] [--size 16] [--dims 4 64]

One process, one context.  Per dim: a round of groups x size clients under the harness's simulated
keys (hashed on the GPU), every client's peers the others of its group.  The two routes' bytes are
compared first; then they are timed alternately, three times each (wall time of the whole call,
uploads and downloads included; the old route split into its three parts), and the fused kernel's
own time is read from the profiler for several chunk_terms.  Prints one JSON line per dim
(DESIGN.md §18 quotes them).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "verifiable-federated-training-with-zero-knowledge-proofs-zk-fl-_amd")]

from zkfl import native, secagg  # noqa: E402
from zkfl.field import R  # noqa: E402

RND = 7
CHUNKS = (1, 2, 3, 4, 5, 8, 15, 0)


def _note(msg):
    print(f"[bench_secagg] {msg}", file=sys.stderr, flush=True)


def _u64_rows(cols):
    """Columns of unsigned 64-bit integers -> (n, len(cols), 32) uint8 field elements."""
    rows = np.zeros((len(cols[0]), len(cols), 4), np.uint64)
    for c, v in enumerate(cols):
        rows[:, c, 0] = v
    return rows.astype("<u8").view(np.uint8).reshape(len(cols[0]), len(cols), 32)


def old_route(ctx, own, peer, keys, grads_int, dim, n, peers_each):
    """-> (masked bytes, [host rows s, poseidon_batch s, host sums s])"""
    t0 = time.perf_counter()
    T = len(own)
    rows = np.zeros((T, dim, 5, 32), np.uint8)
    rows[:, :, 0, :] = keys[:, None, :]
    rows[:, :, 1, 0] = RND
    rows[:, :, 2, :] = _u64_rows([np.minimum(own, peer)])[:, None, 0, :]
    rows[:, :, 3, :] = _u64_rows([np.maximum(own, peer)])[:, None, 0, :]
    rows[:, :, 4, :] = _u64_rows([np.arange(dim, dtype=np.uint64)])[None, :, 0, :]
    t1 = time.perf_counter()
    h = ctx.poseidon_batch_raw(5, rows)
    t2 = time.perf_counter()
    hb = h.tobytes()
    hi = np.array([int.from_bytes(hb[i:i + 32], "little") for i in range(0, len(hb), 32)], dtype=object)
    hi = hi.reshape(n, peers_each, dim)
    sign = np.where(own < peer, 1, -1).astype(object).reshape(n, peers_each, 1)
    masked = ((hi * sign).sum(axis=1) + grads_int) % R
    out = b"".join(int(v).to_bytes(32, "little") for v in masked.reshape(-1))
    t3 = time.perf_counter()
    return out, [t1 - t0, t2 - t1, t3 - t2]


def bench(ctx, groups, size, dim):
    n, pe = groups * size, size - 1
    rng = np.random.default_rng(dim)
    ids = np.arange(1, n + 1, dtype=np.uint64)
    grads = rng.integers(-10 ** 6, 10 ** 6, size=(n, dim), dtype=np.int64)
    g = ids.reshape(groups, size)
    keep = ~np.eye(size, dtype=bool)
    own = np.repeat(g[:, :, None], size, axis=2)[:, keep].reshape(-1)
    peer = np.repeat(g[:, None, :], size, axis=1)[:, keep].reshape(-1)
    keys = secagg.harness_keys(ctx, np.stack([own, peer], axis=1))
    ptr = np.arange(n + 1, dtype=np.uint64) * np.uint64(pe)
    gb = secagg.fr_bytes(grads)
    grads_int = grads.astype(object)
    hashes = len(own) * dim
    out = {"groups": groups, "group_size": size, "dim": dim, "clients": n, "hashes": hashes}

    fused = ctx.secagg_mask(ids, ptr, peer, keys, RND, gb, dim).tobytes()
    old, _ = old_route(ctx, own, peer, keys, grads_int, dim, n, pe)
    assert fused == old, "the two routes disagree"
    _note(f"dim {dim}: {hashes} hashes, the two routes' bytes are equal")

    tf, to, parts = [], [], []
    for _ in range(3):
        t0 = time.perf_counter()
        ctx.secagg_mask(ids, ptr, peer, keys, RND, gb, dim)
        tf.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        _, p = old_route(ctx, own, peer, keys, grads_int, dim, n, pe)
        to.append(time.perf_counter() - t0)
        parts.append(p)
        _note(f"dim {dim}: fused {1e3 * tf[-1]:.2f} ms, old route {1e3 * to[-1]:.1f} ms "
              f"(rows {1e3 * p[0]:.1f}, poseidon_batch {1e3 * p[1]:.1f}, sums {1e3 * p[2]:.1f})")
    out["fused_ms"] = [round(1e3 * t, 3) for t in tf]
    out["old_route_ms"] = [round(1e3 * t, 1) for t in to]
    out["old_route_parts_ms"] = {k: round(1e3 * statistics.median(p[i] for p in parts), 1)
                                 for i, k in enumerate(("host_rows", "poseidon_batch", "host_sums"))}
    out["ratio"] = round(statistics.median(to) / statistics.median(tf), 1)
    out["fused_hashes_per_s"] = round(hashes / statistics.median(tf))

    ctx.set_profiling(True)
    kern = {}
    for ct in CHUNKS:
        ms = []
        for _ in range(3):
            ctx.profile_reset()
            ctx.secagg_mask(ids, ptr, peer, keys, RND, gb, dim, chunk_terms=ct)
            ms.append(ctx.profile("secagg_terms")[0])
        fold = ctx.profile("secagg_fold")[0]
        kern[str(ct)] = {"terms_ms": round(statistics.median(ms), 3), "fold_ms": round(fold, 3),
                         "hashes_per_s": round(hashes / (1e-3 * statistics.median(ms)))}
        _note(f"dim {dim}: chunk_terms {ct}: secagg_terms {kern[str(ct)]['terms_ms']} ms, fold {fold:.3f} ms")
    ctx.profile_reset()
    ctx.set_profiling(False)
    out["kernel_by_chunk_terms"] = kern
    return out


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--groups", type=int, default=128)
    ap.add_argument("--size", type=int, default=16)
    ap.add_argument("--dims", type=int, nargs="+", default=[4, 64])
    a = ap.parse_args(argv)
    with native.Context(0) as ctx:
        _note(f"libzkfl build {native.build_id()}")
        ctx.secagg_mask([1], [0, 1], [2], (5).to_bytes(32, "little"), RND, bytes(32), 1)   # warm-up: tables, code
        for dim in a.dims:
            print(json.dumps(bench(ctx, a.groups, a.size, dim)), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
