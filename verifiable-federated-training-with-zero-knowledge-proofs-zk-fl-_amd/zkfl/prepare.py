"""Preparing a round: every client's three input.json files, computed on the GPU in one call.

The reference's clients compute, before they prove (tests/full_system_simulation.mjs:1278-1343): the
dataset tree and its Merkle openings (computeDatasetCommitment :308-335, getMerkleProof :225-238), the
fixed-point gradient with its floor division (_computeVerifiedGradient :511-553), gradPos / gradNeg
and the clipping test (:411-431), the commitments root_W, root_G, root_K and the masked update
(:433-438, :565-609).  zkfl/clients.py restates that one client at a time with the Python Poseidon and
stays the model; `prepare_round` does it for all clients of a round in one call of the library
(zkfl_round_prepare, csrc/prepare.hip) and returns the circuits' flat input vectors, ready for
ProvingKey.full_prove_batch, and the fields of the clients' packages (zkfl/admit.py).

A spec is a dict:
    "ids":        the clients' ids (distinct unsigned 64-bit integers),
    "samples", "dim", "depth", "batch", "precision": the shape, the same for every client,
    "features":   n x samples x dim signed integers (a negative x stands for r - |x|),
    "labels":     n x samples, each 0 or 1,
    "batch_idx":  n x batch sample indices (optional: 0..batch-1, the reference's choice),
    "weights":    dim signed integers, the global model,
    "round", "tau_squared": the round (a field element) and the clipping bound (< 2^64 - 1),
    "peers":      n lists of peer ids, all of one length 0..15 (optional or empty: no secagg part),
    "keys":       n lists of pairwise keys aligned with "peers" (field elements),
    "master_keys": n field elements.
Key agreement stays the caller's protocol; `harness_keys` gives the harness's simulated keys.
`pack` raises ValueError, before anything touches the GPU, for every spec the library would refuse.
"""

from __future__ import annotations

import numpy as np

from . import native
from .field import R, poseidon_hash
from .secagg import HARNESS_KEY_SALT, fr_bytes, signed

PHASES = native.ADMIT_PHASES
STATUS = {native.PREPARE_OK: "OK", native.PREPARE_NORM: "NORM"}
I64_MAX = (1 << 63) - 1


def _int_array(values, shape, what, lo, hi, dtype):
    if isinstance(values, np.ndarray) and values.dtype.kind in "iu":      # no Python loop over a large round
        if values.shape != shape:
            raise ValueError(f"{what} must have the shape {shape}, not {values.shape}")
        if values.size and not (lo <= int(values.min()) and int(values.max()) <= hi):
            raise ValueError(f"{what}: a value is outside {lo}..{hi}")
        return np.ascontiguousarray(values.astype(dtype, copy=False))
    try:
        arr = np.asarray(values, dtype=object)
        if arr.shape != shape:
            raise ValueError(f"{what} must have the shape {shape}, not {arr.shape}")
        flat = [int(v) for v in arr.reshape(-1)]
    except TypeError as e:
        raise ValueError(f"{what}: {e}") from None
    for k, v in enumerate(flat):
        if not lo <= v <= hi:
            raise ValueError(f"{what}: entry {k} = {v} is outside {lo}..{hi}")
    return np.array(flat, dtype=dtype).reshape(shape)


def _fr(v, what) -> int:
    x = int(v)
    if not 0 <= x < R:
        raise ValueError(f"{what}: {x} is not a canonical field element (not < r)")
    return x


def pack(spec: dict) -> dict:
    """A spec -> the arrays of Context.round_prepare (host only).  Raises ValueError for what
    zkfl_round_prepare refuses with ZKFL_E_ARG, naming the client or index."""
    try:
        ids = [int(c) for c in spec["ids"]]
        S, dim, depth, batch, precision = (int(spec[k]) for k in ("samples", "dim", "depth", "batch", "precision"))
        tau = int(spec["tau_squared"])
        rnd = int(spec["round"])
    except (KeyError, TypeError) as e:
        raise ValueError(f"spec: {e!r}") from None
    n = len(ids)
    if len(set(ids)) != n or not all(0 <= c < 1 << 64 for c in ids):
        raise ValueError("spec: client ids must be distinct unsigned 64-bit integers")
    if not 1 <= dim <= native.PREPARE_MAX_DIM:
        raise ValueError(f"dim {dim} must be in 1..{native.PREPARE_MAX_DIM}: a leaf has dim + 1 <= 256 values")
    if not 1 <= depth <= native.MERKLE_MAX_DEPTH:
        raise ValueError(f"depth {depth} must be in 1..{native.MERKLE_MAX_DEPTH}")
    if not 1 <= S <= 1 << depth:
        raise ValueError(f"samples {S} must be in 1..2^depth = {1 << depth}")
    if not 1 <= batch <= S:
        raise ValueError(f"batch {batch} must be in 1..samples = {S}")
    if not 1 <= precision < 1 << 32:
        raise ValueError("precision must be in 1..2^32 - 1")
    if not 0 <= tau < (1 << 64) - 1:
        raise ValueError("tau_squared must be in 0..2^64 - 2: the circuit's LessThan(64) takes tau_squared + 1")
    _fr(rnd, "round")
    peers = spec.get("peers")
    peers = [] if peers is None else peers
    if len(peers) not in (0, n):
        raise ValueError("peers must hold one list per client")
    counts = {len(p) for p in peers}
    if len(counts) > 1:
        raise ValueError("every client must have the same number of peers")
    np_ = counts.pop() if counts else 0
    if np_ > native.PREPARE_MAX_PEERS:
        raise ValueError(f"peers {np_} must be at most {native.PREPARE_MAX_PEERS}: root_K is one Poseidon of peers + 1 inputs")
    if np_ == 0 and any(spec.get(k) is not None and len(spec[k]) for k in ("keys", "master_keys")):
        raise ValueError("peers == 0 means no secagg part: keys and master_keys must be absent")

    features = _int_array(spec["features"], (n, S, dim), "features", -(1 << 63), I64_MAX, np.int64)
    labels = np.asarray(_int_array(spec["labels"], (n, S), "labels", 0, 255, np.uint8))
    for i, s in zip(*np.nonzero(labels > 1)):
        raise ValueError(f"client {i}: label {s} is {labels[i, s]}, not 0 or 1")
    weights = _int_array(spec["weights"], (dim,), "weights", -(1 << 63), I64_MAX, np.int64)
    out = {"ids": np.array(ids, dtype=np.uint64), "samples": S, "dim": dim, "depth": depth, "batch": batch,
           "precision": precision, "peers": np_, "features": features, "labels": labels, "weights": weights,
           "round": rnd, "tau_squared": tau, "batch_idx": None}
    if spec.get("batch_idx") is not None:
        idx = _int_array(spec["batch_idx"], (n, batch), "batch_idx", 0, (1 << 32) - 1, np.uint32)
        for i, b in zip(*np.nonzero(idx >= S)):
            raise ValueError(f"client {i}: batch_idx {b} is {idx[i, b]}, samples is {S}")
        out["batch_idx"] = idx
    if np_:
        pid = _int_array(peers, (n, np_), "peers", 0, (1 << 64) - 1, np.uint64)
        try:
            keys, masters = spec["keys"], spec["master_keys"]
            if len(keys) != n or len(masters) != n or any(len(k) != np_ for k in keys):
                raise ValueError("keys must hold one key per peer and master_keys one key per client")
        except (KeyError, TypeError):
            raise ValueError("peers > 0 needs keys and master_keys") from None
        for i in range(n):
            lst = [int(x) for x in pid[i]]
            for j, p in enumerate(lst):
                if p == ids[i]:
                    raise ValueError(f"client {i}: peer {j} is the client's own id")
                if p in lst[:j]:
                    raise ValueError(f"client {i}: peer {j} repeats peer {lst.index(p)}")
        if isinstance(keys, np.ndarray) and keys.dtype == np.uint8:
            kb = fr_bytes(keys).reshape(n, np_, 32)
            big = [(i, j) for i in range(n) for j in range(np_) if int.from_bytes(kb[i, j].tobytes(), "little") >= R]
            if big:
                raise ValueError(f"client {big[0][0]}: key {big[0][1]} is not < r")
        else:
            kb = fr_bytes([[_fr(k, f"client {i}: key {j}") for j, k in enumerate(row)] for i, row in enumerate(keys)])
        if isinstance(masters, np.ndarray) and masters.dtype == np.uint8:
            mb = fr_bytes(masters).reshape(n, 32)
            for i in range(n):
                _fr(int.from_bytes(mb[i].tobytes(), "little"), f"client {i}: master key")
        else:
            mb = fr_bytes([_fr(m, f"client {i}: master key") for i, m in enumerate(masters)])
        out.update(peer_ids=pid, keys=kb.reshape(n, np_, 32), master_keys=mb.reshape(n, 32))
    # the overflow bound, in Python integers: batch * F * (dim * F * W + precision) <= 2^63 - 1
    F = max(abs(int(features.max())), abs(int(features.min()))) if features.size else 0
    W = max(abs(int(x)) for x in weights)
    bound = batch * F * (dim * F * W + precision)
    if bound > I64_MAX:
        raise ValueError(f"overflow bound: batch * F * (dim * F * W + precision) = {bound} exceeds 2^63 - 1 "
                         f"(F = {F}, W = {W})")
    return out


def harness_dataset(client_id: int, samples: int, dim: int, seed: int | None = None):
    """The harness's private dataset of one client (tests/full_system_simulation.mjs:273-303;
    zkfl/clients.py::Client without its tree): features 0..100 from the seeded LCG, labels
    alternating from the id.  seed: the LCG's seed (default 12345 + id, as clients.federated_round)."""
    from .clients import JsLcg
    lcg = JsLcg(12345 + client_id if seed is None else seed)
    feats = [[lcg.randint(0, 100, client_id * 1000 + i * 10 + j) for j in range(dim)] for i in range(samples)]
    return feats, [(i + client_id) % 2 for i in range(samples)]


def harness_keys(ids, group_size: int | None = None):
    """The harness's simulated key agreement on the host (tests/full_system_simulation.mjs:1321-1336):
    ids cut into consecutive groups, every client's peers the others of its group, K_ij =
    Poseidon(min, max, 12345) and the master key Poseidon(id, 12345).  -> (peers, keys, master_keys).
    For thousands of clients hash the pairs on the GPU instead (zkfl/secagg.py::harness_keys)."""
    ids = [int(c) for c in ids]
    gs = len(ids) if group_size is None else int(group_size)
    if ids and (gs < 1 or len(ids) % gs):
        raise ValueError("group_size must divide the number of clients")
    peers = [[p for p in ids[i - i % gs:i - i % gs + gs] if p != c] for i, c in enumerate(ids)]
    keys = [[poseidon_hash([min(c, p), max(c, p), HARNESS_KEY_SALT]) for p in lst] for c, lst in zip(ids, peers)]
    return peers, keys, [poseidon_hash([c, HARNESS_KEY_SALT]) for c in ids]


def _ints(row) -> list:
    b = np.ascontiguousarray(row).tobytes()
    return [int.from_bytes(b[k:k + 32], "little") for k in range(0, len(b), 32)]


class Prepared:
    """prepare_round's result.  `inputs[phase]`: uint8 (n, n_inputs, 32), the circuit's input vectors
    (inputs["secagg"] only with peers); `status` (uint32 n, native.PREPARE_*), `gradients` (int64 n x
    dim), `roots` (uint8 n x 4 x 32: D, G, W, K), `masked` (uint8 n x dim x 32 or None), `c1`."""

    def __init__(self, packed: dict, res: dict):
        self.packed = packed
        self.ids = [int(c) for c in packed["ids"]]
        self.inputs = {p: res[f"{p}_inputs"] for p in PHASES if f"{p}_inputs" in res}
        self.status, self.gradients, self.roots = res["status"], res["gradients"], res["roots"]
        self.masked, self.c1 = res.get("masked"), res["c1"]

    @property
    def ok(self) -> bool:
        return not self.status.any()

    def _batch_rows(self, i):
        a = self.packed
        return list(range(a["batch"])) if a["batch_idx"] is None else [int(x) for x in a["batch_idx"][i]]

    def input_json(self, phase: str, i: int) -> dict:
        """Client i's input.json of a phase, shaped as the reference's (and zkfl/clients.py's): decimal
        strings; features, weights and expectedSummedGrad signed, every other value a field element."""
        a = self.packed
        S, dim, depth, batch, peers = a["samples"], a["dim"], a["depth"], a["batch"], a["peers"]
        v = [str(x) for x in _ints(self.inputs[phase][i])]

        def grid(flat, cols):
            return [flat[r * cols:(r + 1) * cols] for r in range(len(flat) // cols)]

        if phase == "balance":
            o = 5 + S * dim + S
            return {"client_id": v[0], "root": v[1], "N_public": v[2], "c0": v[3], "c1": v[4],
                    "features": [[str(int(x)) for x in row] for row in a["features"][i]],
                    "labels": v[5 + S * dim:o], "siblings": grid(v[o:o + S * depth], depth),
                    "pathIndices": grid(v[o + S * depth:], depth)}
        if phase == "training":
            o = 6 + 5 * dim
            q = o + batch * dim + batch
            return {"client_id": v[0], "round": v[1], "root_D": v[2], "root_G": v[3], "root_W": v[4],
                    "tauSquared": v[5], "weights": [str(int(w)) for w in a["weights"]],
                    "expectedSummedGrad": [str(signed(int(x))) for x in v[6 + dim:6 + 2 * dim]],
                    "remainder": v[6 + 2 * dim:6 + 3 * dim], "gradPos": v[6 + 3 * dim:6 + 4 * dim],
                    "gradNeg": v[6 + 4 * dim:o],
                    "features": [[str(int(x)) for x in a["features"][i][r]] for r in self._batch_rows(i)],
                    "labels": v[o + batch * dim:q], "siblings": grid(v[q:q + batch * depth], depth),
                    "pathIndices": grid(v[q + batch * depth:], depth)}
        if phase == "secagg":
            o = 7 + dim
            return {"client_id": v[0], "round": v[1], "root_D": v[2], "root_G": v[3], "root_W": v[4],
                    "root_K": v[5], "tauSquared": v[6], "masked_update": v[7:o], "peer_ids": v[o:o + peers],
                    "gradient": v[o + peers:o + peers + dim], "master_key": v[o + peers + dim],
                    "shared_keys": v[o + peers + dim + 1:]}
        raise KeyError(phase)

    def round(self, proofs: dict, vkeys: dict, clients=None) -> dict:
        """The round dict of admit.admit_round.  proofs: {phase: [(proof, public signals)] in client
        order} as ProvingKey.full_prove_batch returns them (a phase may be absent); vkeys: {phase:
        vkey.json dict or VerifyingKey}.  clients: the ids to include (default: all)."""
        a = self.packed
        roots = [_ints(r) for r in self.roots]
        rnd = {"round": a["round"], "tau_squared": a["tau_squared"], "dim": a["dim"], "vkeys": vkeys,
               "clients": list(self.ids) if clients is None else [int(c) for c in clients],
               "weights": [int(w) % R for w in a["weights"]], "balance": {}, "training": {}, "secagg": {}}
        if a["peers"]:
            rnd["peers"] = {cid: [int(p) for p in a["peer_ids"][i]] for i, cid in enumerate(self.ids)}
        for i, cid in enumerate(self.ids):
            if cid not in rnd["clients"]:
                continue
            d, g, w, k = roots[i]
            fields = {"balance": {"root_D": d},
                      "training": {"root_D": d, "root_G": g, "root_W": w, "round": a["round"],
                                   "gradient": [int(x) for x in self.gradients[i]]},
                      "secagg": {"root_D": d, "root_G": g, "root_W": w, "root_K": k, "round": a["round"],
                                 "masked_update": _ints(self.masked[i]) if self.masked is not None else []}}
            for p in PHASES:
                if proofs.get(p) is None:
                    continue
                proof, pub = proofs[p][i]
                rnd[p][cid] = dict(fields[p], proof=proof, publicSignals=[int(x) for x in pub])
        return rnd


def prepare_round(ctx, spec: dict, want=None, packed: dict | None = None) -> Prepared:
    """Prepare a round on `ctx` (native.Context) -> Prepared.  want: the outputs to compute
    (native.PREPARE_OUTPUTS; None: all the shape has).  packed: pack(spec), when already validated."""
    a = packed if packed is not None else pack(spec)
    return Prepared(a, ctx.round_prepare(a, want))
