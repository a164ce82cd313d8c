"""Admitting a round: which clients' updates may enter the aggregate, and why not the others.

The reference's server decides this in three methods of its `Server` class
(tests/full_system_simulation.mjs: verifyBalanceProof :848-880, verifyTrainingProof :886-990,
verifySecureAggregationProof :995-1131): before each `groth16 verify` it compares the public
signals with the fields the client claimed, binds the client's three proofs to each other through
root_D, root_G and root_W, holds tauSquared to its clipping bound and recomputes root_G from the
submitted gradient; and it takes no training proof without an accepted balance proof, no secagg
proof without an accepted training proof.  `admit_round` runs all of that for a whole round in one
call of the library (zkfl_round_admit, csrc/admit.hip) and returns one code per client and phase:
0, or the first failing check (include/zkfl.h, ZKFL_ADMIT_*; names in native.ADMIT_CODES).

A round is a dict:
    "round", "tau_squared": the server's round and clipping bound,
    "dim":      the model dimension,
    "clients":  the ids, in the order the results are reported,
    "vkeys":    {"balance", "training", "secagg"}: vkey.json dicts (or Prover.load_vkey handles),
    "balance":  {id: proofPackage}   {"proof", "publicSignals", "root_D"}                  (:387-394)
    "training": {id: updatePackage}  {"proof", "publicSignals", "root_D", "root_G", "root_W", "round",
                                      "gradient": dim signed integers}                     (:494-505)
    "secagg":   {id: secaggPackage}  {"proof", "publicSignals", "root_D", "root_G", "root_W", "root_K",
                                      "round", "masked_update": dim values}                (:657-667)
    "weights":  the global model, dim values (optional: the model check needs it),
    "peers":    {id: [peer ids]} in the order of the circuit's peer_ids (optional: the peer check).
A client without an entry in a phase's dict has no package there.  Values are integers or decimal
strings; `pack` raises ValueError, before anything touches the GPU, for one that is not a canonical
field element (0 <= v < r), a gradient outside int64, an id outside uint64 or a package of the
wrong shape.
"""

from __future__ import annotations

import numpy as np

from . import native
from .field import R

PHASES = native.ADMIT_PHASES
ALL_CHECKS = native.ADMIT_CHECK_ROUND | native.ADMIT_CHECK_MODEL | native.ADMIT_CHECK_PEERS


def code_name(code: int) -> str:
    return native.ADMIT_CODES.get(int(code), f"code {int(code)}")


def accepted(codes: dict) -> list:
    """The clients whose secagg code is 0: those the reference puts into `secaggUpdates` (:1127)."""
    return [cid for cid, c in codes.items() if c[2] == 0]


def _fr(v, what) -> int:
    try:
        x = int(v)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: {v!r} is not an integer") from None
    if isinstance(v, str) and v != str(x):
        raise ValueError(f"{what}: {v!r} is not a canonical decimal string")
    if not 0 <= x < R:
        raise ValueError(f"{what}: {x} is not a canonical field element")
    return x


def _frs(values) -> np.ndarray:
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in values), dtype=np.uint8)


def pack(rnd: dict, proofs: bool = True) -> dict:
    """A round dict -> the flat arrays of Context.round_admit (host only).  proofs False: packages
    need no "proof" (the static parity hook).  The result also carries "secagg_npublic" (None when
    no client sent a secagg package)."""
    from . import groth16
    try:
        ids = [int(c) for c in rnd["clients"]]
        dim = int(rnd["dim"])
        phases = {p: rnd.get(p) or {} for p in PHASES}
    except (KeyError, TypeError, ValueError) as e:
        raise ValueError(f"round: {e!r}") from None
    if len(set(ids)) != len(ids) or not all(0 <= c < 1 << 64 for c in ids):
        raise ValueError("round: client ids must be distinct unsigned 64-bit integers")
    if not 1 <= dim <= 256:
        raise ValueError("round: dim must be in 1..256")
    n = len(ids)
    out = {"ids": np.array(ids, dtype=np.uint64), "dim": dim, "round": _fr(rnd.get("round"), "round"),
           "tau_squared": _fr(rnd.get("tau_squared"), "tau_squared")}
    grads = np.zeros((n, dim), np.int64)
    masked = [0] * (n * dim)
    s_npub = None
    for p in PHASES:
        fields = native.ADMIT_FIELDS[p]
        stray = [c for c in phases[p] if int(c) not in ids]
        if stray:
            raise ValueError(f"{p}: package of client {stray[0]}, which is not in the round")
        pk = {int(c): v for c, v in phases[p].items()}
        present = np.zeros(n, np.uint8)
        npub = native.ADMIT_NPUBLIC[p]
        if p == "secagg":
            counts = {len(v.get("publicSignals", ())) for v in pk.values() if isinstance(v, dict)}
            if len(counts) > 1:
                raise ValueError("secagg: the packages have public signals of different lengths")
            npub = s_npub = counts.pop() if counts else None
            if npub is not None and npub < 7 + dim:
                raise ValueError(f"secagg: {npub} public signals, dim {dim} needs at least {7 + dim}")
        claimed, signals, prf = [], [], []
        for i, cid in enumerate(ids):
            v = pk.get(cid)
            who = f"client {cid} {p}"
            if v is None:
                claimed += [0] * len(fields)
                signals += [0] * (npub or 0)
                prf.append(bytes(256))
                continue
            if not isinstance(v, dict):
                raise ValueError(f"{who}: a package must be an object")
            present[i] = 1
            try:
                sig = list(v["publicSignals"])
                claimed += [_fr(v[f], f"{who} {f}") for f in fields]
                if p == "training":
                    g = [int(x) for x in v["gradient"]]
                    if len(g) != dim or not all(-(1 << 63) <= x < 1 << 63 for x in g):
                        raise ValueError(f"{who}: gradient must be {dim} signed 64-bit integers")
                    grads[i] = g
                if p == "secagg":
                    m = [_fr(x, f"{who} masked_update") for x in v["masked_update"]]
                    if len(m) != dim:
                        raise ValueError(f"{who}: masked_update must hold {dim} values")
                    masked[i * dim:(i + 1) * dim] = m
                if proofs:
                    pr = v["proof"]
                    prf.append(bytes(pr) if isinstance(pr, (bytes, bytearray)) else groth16.proof_from_json(pr))
                    if len(prf[-1]) != 256:
                        raise ValueError(f"{who}: a proof is 256 bytes")
            except KeyError as e:
                raise ValueError(f"{who}: no field {e}") from None
            except (TypeError, AssertionError) as e:
                raise ValueError(f"{who}: {e}") from None
            if len(sig) != npub:
                raise ValueError(f"{who}: {len(sig)} public signals, expected {npub}")
            signals += [_fr(x, f"{who} public signal {k}") for k, x in enumerate(sig)]
        out[p] = {"present": present, "claimed": _frs(claimed) if present.any() else None,
                  "signals": _frs(signals) if present.any() else None,
                  "proofs": np.frombuffer(b"".join(prf), dtype=np.uint8) if proofs and present.any() else None}
    out["gradients"] = grads
    out["masked_update"] = _frs(masked)
    out["secagg_npublic"] = s_npub
    if rnd.get("weights") is not None:
        w = [_fr(x, f"weight {k}") for k, x in enumerate(rnd["weights"])]
        if len(w) != dim:
            raise ValueError(f"round: weights must hold {dim} values")
        out["weights"] = _frs(w)
    if rnd.get("peers") is not None:
        try:
            lists = [[int(x) for x in rnd["peers"].get(cid, rnd["peers"].get(str(cid), ()))] for cid in ids]
        except (TypeError, ValueError, AttributeError) as e:
            raise ValueError(f"round: peers: {e}") from None
        if not all(0 <= x < 1 << 64 for lst in lists for x in lst):
            raise ValueError("round: a peer id is not an unsigned 64-bit integer")
        ptr = np.zeros(n + 1, np.uint64)
        np.cumsum([len(lst) for lst in lists], out=ptr[1:])
        out["peer_ptr"] = ptr
        out["peer_ids"] = np.array([x for lst in lists for x in lst], dtype=np.uint64)
    return out


def flags_for(rnd: dict, reference: bool = False, combined: bool = False) -> int:
    """The flags of a round: the three added checks unless `reference`, each only when the round
    carries its input (the model check needs "weights", the peer check "peers")."""
    flags = native.ADMIT_COMBINED if combined else 0
    if not reference:
        flags |= native.ADMIT_CHECK_ROUND
        if rnd.get("weights") is not None:
            flags |= native.ADMIT_CHECK_MODEL
        if rnd.get("peers") is not None:
            flags |= native.ADMIT_CHECK_PEERS
    return flags


class Admission:
    """admit_round's result: `codes` {id: (balance, training, secagg)}, `report` (the verifier's),
    `names` the same with the codes' names, `accepted` the ids whose secagg code is 0."""

    def __init__(self, ids, codes, report):
        self.codes = {cid: tuple(int(codes[p][i]) for p in range(3)) for i, cid in enumerate(ids)}
        self.report = report

    @property
    def names(self) -> dict:
        return {cid: tuple(code_name(c) for c in cs) for cid, cs in self.codes.items()}

    @property
    def accepted(self) -> list:
        return accepted(self.codes)


def admit_round(prover, rnd: dict, reference: bool = False, combined: bool = False, packed: dict | None = None,
                flags: int | None = None) -> Admission:
    """Admit a round on `prover` (groth16.Prover) -> Admission.  reference: only the reference's
    checks; combined: the proofs go to the round verifier.  packed: pack(rnd), when the caller has
    validated the round already."""
    a = packed if packed is not None else pack(rnd)
    vks = [k if isinstance(k, native.VerifyingKey) else prover.load_vkey(k) for k in (rnd["vkeys"][p] for p in PHASES)]
    if a["secagg_npublic"] not in (None, vks[2].n_public):
        raise ValueError(f"secagg: the packages have {a['secagg_npublic']} public signals, the key "
                         f"{vks[2].n_public}")
    codes, rep = prover.ctx.round_admit(a, vks, flags_for(rnd, reference, combined) if flags is None else flags)
    return Admission([int(c) for c in a["ids"]], codes, rep)
