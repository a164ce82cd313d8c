"""Plain-Python model of the reference server's admission checks, for the admit tests.

`Server` restates the three methods of the reference's Server class
(tests/full_system_simulation.mjs: verifyBalanceProof :848-880, verifyTrainingProof :886-990,
verifySecureAggregationProof :995-1131) over package dicts, statement by statement and in the
reference's order; the proof verdicts come from a callback.  Each of the three additions
(include/zkfl.h: ZKFL_ADMIT_CHECK_ROUND / _MODEL / _PEERS) has a switch.  `admit` runs a round
through it; `synthetic_round` makes an honest round without circuits or proofs; TAMPERS turns an
honest round into one where exactly one check fails first for one client.
"""
import copy
import functools
import random

from zkfl import clients
from zkfl.field import R
from zkfl.native import ADMIT_CODES

C = {name: code for code, name in ADMIT_CODES.items()}   # "T_SIG_TAU" -> 24
INT64_MAX, INT64_MIN = (1 << 63) - 1, -(1 << 63)


@functools.lru_cache(maxsize=None)
def _vector_hash(values: tuple) -> int:
    return clients.vector_hash(values)


@functools.lru_cache(maxsize=None)
def gradient_commitment(grad: tuple, client_id: int, rnd: int) -> int:
    """gradientCommitment (:159-164) over the signed gradient (:955)."""
    field = tuple(g if g >= 0 else R + g for g in grad)
    return clients.poseidon_hash([_vector_hash(field), clients.poseidon_hash([client_id, rnd])])


def weight_commitment(weights) -> int:
    return _vector_hash(tuple(int(w) for w in weights))


class Server:
    def __init__(self, rnd, tau_squared, verdict, check_round=False, weights=None, peers=None):
        """verdict(phase, client id, package) -> bool.  check_round: the CHECK_ROUND addition;
        weights not None: CHECK_MODEL; peers ({id: [ids]}) not None: CHECK_PEERS."""
        self.round, self.tau, self.verdict = int(rnd), int(tau_squared), verdict
        self.check_round, self.weights, self.peers = check_round, weights, peers
        self.balance_proofs, self.training_updates, self.secagg_updates = {}, {}, {}

    def verify_balance(self, cid, p):
        if p is None:
            return C["B_MISSING"]
        if int(p["publicSignals"][1]) != int(p["root_D"]):
            return C["B_SIG_ROOT_D"]
        if not self.verdict("balance", cid, p):
            return C["B_PROOF"]
        self.balance_proofs[cid] = p
        return 0

    def verify_training(self, cid, p):
        if p is None:
            return C["T_MISSING"]
        sig = [int(x) for x in p["publicSignals"]]
        bal = self.balance_proofs.get(cid)
        if bal is None:
            return C["T_NO_BALANCE"]
        if int(p["root_D"]) != int(bal["root_D"]):
            return C["T_BIND_ROOT_D"]
        if sig[2] != int(p["root_D"]):
            return C["T_SIG_ROOT_D"]
        if sig[3] != int(p["root_G"]):
            return C["T_SIG_ROOT_G"]
        if sig[4] != int(p["root_W"]):
            return C["T_SIG_ROOT_W"]
        if sig[1] != int(p["round"]):
            return C["T_SIG_ROUND"]
        if self.check_round and int(p["round"]) != self.round:
            return C["T_ROUND_STALE"]
        if sig[5] != self.tau:
            return C["T_SIG_TAU"]
        if gradient_commitment(tuple(int(g) for g in p["gradient"]), cid, int(p["round"])) != int(p["root_G"]):
            return C["T_ROOT_G_GRADIENT"]
        if self.weights is not None and int(p["root_W"]) != weight_commitment(self.weights):
            return C["T_ROOT_W_MODEL"]
        if not self.verdict("training", cid, p):
            return C["T_PROOF"]
        self.training_updates[cid] = p
        return 0

    def verify_secagg(self, cid, p):
        if p is None:
            return C["S_MISSING"]
        sig = [int(x) for x in p["publicSignals"]]
        trn = self.training_updates.get(cid)
        if trn is None:
            return C["S_NO_TRAINING"]
        if int(p["root_G"]) != int(trn["root_G"]):
            return C["S_BIND_ROOT_G"]
        bal = self.balance_proofs[cid]          # :1018-1023 cannot fire: the training proof was accepted
        if int(p["root_D"]) != int(bal["root_D"]):
            return C["S_BIND_ROOT_D"]
        if int(p["root_W"]) != int(trn["root_W"]):
            return C["S_BIND_ROOT_W"]
        if sig[0] != cid:
            return C["S_SIG_CLIENT_ID"]
        if sig[1] != int(p["round"]):
            return C["S_SIG_ROUND"]
        if self.check_round and int(p["round"]) != self.round:
            return C["S_ROUND_STALE"]
        for k, (field, code) in enumerate((("root_D", "S_SIG_ROOT_D"), ("root_G", "S_SIG_ROOT_G"),
                                           ("root_W", "S_SIG_ROOT_W"), ("root_K", "S_SIG_ROOT_K"))):
            if sig[2 + k] != int(p[field]):
                return C[code]
        if sig[6] != self.tau:
            return C["S_SIG_TAU"]
        dim = len(p["masked_update"])
        if any(sig[7 + k] != int(m) for k, m in enumerate(p["masked_update"])):
            return C["S_SIG_MASKED"]
        if self.peers is not None and sig[7 + dim:] != [int(x) for x in self.peers.get(cid, ())]:
            return C["S_SIG_PEERS"]
        if not self.verdict("secagg", cid, p):
            return C["S_PROOF"]
        self.secagg_updates[cid] = p
        return 0


def admit(rnd, verdict=lambda phase, cid, p: True, check_round=True, check_model=True, check_peers=True):
    """{id: (balance, training, secagg)}: the three phases in the reference's order (:1298-1343)."""
    s = Server(rnd["round"], rnd["tau_squared"], verdict, check_round,
               rnd.get("weights") if check_model else None, rnd.get("peers") if check_peers else None)
    ids = [int(c) for c in rnd["clients"]]
    b = [s.verify_balance(c, rnd["balance"].get(c)) for c in ids]
    t = [s.verify_training(c, rnd["training"].get(c)) for c in ids]
    g = [s.verify_secagg(c, rnd["secagg"].get(c)) for c in ids]
    return {c: (b[i], t[i], g[i]) for i, c in enumerate(ids)}


def fold_static(static):
    """The fold of zkfl_round_admit over the static codes with every proof valid."""
    out = {}
    for cid, (b, t, s) in static.items():
        if t != C["T_MISSING"] and b:
            t = C["T_NO_BALANCE"]
        if s != C["S_MISSING"] and t:
            s = C["S_NO_TRAINING"]
        out[cid] = (b, t, s)
    return out


EDGE_GRADIENTS = (0, 1, -1, INT64_MAX, INT64_MIN, 12345, -98765)


def synthetic_round(n, dim, peers=2, rnd=1, tau_squared=100000000, seed=7):
    """An honest round of n clients without circuits: the signals are what the three circuits
    would publish for these claimed fields; "proof" is a placeholder for the verdict callback."""
    rng = random.Random(seed * 1000003 + n * 257 + dim)
    ids = [1 + i for i in range(n)]
    if n > 2:
        ids[-1] = (1 << 63) + 5                       # an id that needs all 64 bits
    weights = [rng.randrange(R) for _ in range(dim)]
    root_w = weight_commitment(weights)
    out = {"round": rnd, "tau_squared": tau_squared, "dim": dim, "clients": ids, "weights": weights,
           "balance": {}, "training": {}, "secagg": {}, "peers": {}}
    for i, cid in enumerate(ids):
        grad = [EDGE_GRADIENTS[(i + k) % len(EDGE_GRADIENTS)] for k in range(dim)]
        root_d, root_k = rng.randrange(R), rng.randrange(R)
        root_g = gradient_commitment(tuple(grad), cid, rnd)
        masked = [rng.randrange(R) for _ in range(dim)]
        plist = [ids[(i + 1 + j) % n] if n > peers else 1000 + 10 * i + j for j in range(peers)]
        out["peers"][cid] = plist
        out["balance"][cid] = {"proof": "ok", "publicSignals": [cid, root_d, 8, 4, 4], "root_D": root_d}
        out["training"][cid] = {"proof": "ok", "publicSignals": [cid, rnd, root_d, root_g, root_w, tau_squared],
                                "root_D": root_d, "root_G": root_g, "root_W": root_w, "round": rnd, "gradient": grad}
        out["secagg"][cid] = {"proof": "ok",
                              "publicSignals": [cid, rnd, root_d, root_g, root_w, root_k, tau_squared] + masked + plist,
                              "root_D": root_d, "root_G": root_g, "root_W": root_w, "root_K": root_k, "round": rnd,
                              "masked_update": masked}
    return out


def proof_verdict(phase, cid, p):
    return p["proof"] != "bad"


def _bump(p, k):
    p["publicSignals"][k] = (int(p["publicSignals"][k]) + 1) % R


def _bad_proof(phase):
    def f(r, c):
        r[phase][c]["proof"] = "bad"
    return f


def _drop(phase):
    def f(r, c):
        del r[phase][c]
    return f


def _sig(phase, k):
    def f(r, c):
        _bump(r[phase][c], k)
    return f


def _other(v):
    return (int(v) + 12345) % R       # another client's value: any other field element does


def _claim(phase, field, k):
    """The package claims another value and its signal agrees: only the binding can notice."""
    def f(r, c):
        p = r[phase][c]
        p[field] = _other(p[field])
        p["publicSignals"][k] = p[field]
    return f


def _gradient(r, c):
    r["training"][c]["gradient"][0] ^= 1          # stays inside int64 at both ends


def _round_all(r, c):
    """The client runs round + 1 in both packages, consistently (root_G recommitted)."""
    t, s = r["training"][c], r["secagg"][c]
    nr = int(t["round"]) + 1
    g = gradient_commitment(tuple(t["gradient"]), c, nr)
    for p in (t, s):
        p["round"] = nr
        p["publicSignals"][1] = nr
        p["root_G"] = g
        p["publicSignals"][3] = g


def _round_secagg(r, c):
    s = r["secagg"][c]
    s["round"] = int(s["round"]) + 1
    s["publicSignals"][1] = s["round"]


def _model(r, c):
    """The client trained on another model, consistently."""
    w = _other(r["training"][c]["root_W"])
    for p in (r["training"][c], r["secagg"][c]):
        p["root_W"] = w
        p["publicSignals"][4] = w


def _masked_last(r, c):
    _bump(r["secagg"][c], 7 + r["dim"] - 1)


def _peers(r, c):
    sig, d = r["secagg"][c]["publicSignals"], 7 + r["dim"]
    sig[d], sig[d + 1] = sig[d + 1], sig[d]       # a permutation of peer_ids


# name -> (mutation of (round, victim id), the victim's codes with the additions on, the addition it
# needs or None).  With that addition off the victim is accepted (0, 0, 0).
TAMPERS = {
    "B_MISSING": (_drop("balance"), ("B_MISSING", "T_NO_BALANCE", "S_NO_TRAINING"), None),
    "B_SIG_ROOT_D": (_sig("balance", 1), ("B_SIG_ROOT_D", "T_NO_BALANCE", "S_NO_TRAINING"), None),
    "B_PROOF": (_bad_proof("balance"), ("B_PROOF", "T_NO_BALANCE", "S_NO_TRAINING"), None),
    "T_MISSING": (_drop("training"), ("OK", "T_MISSING", "S_NO_TRAINING"), None),
    "T_BIND_ROOT_D": (_claim("training", "root_D", 2), ("OK", "T_BIND_ROOT_D", "S_NO_TRAINING"), None),
    "T_SIG_ROOT_D": (_sig("training", 2), ("OK", "T_SIG_ROOT_D", "S_NO_TRAINING"), None),
    "T_SIG_ROOT_G": (_sig("training", 3), ("OK", "T_SIG_ROOT_G", "S_NO_TRAINING"), None),
    "T_SIG_ROOT_W": (_sig("training", 4), ("OK", "T_SIG_ROOT_W", "S_NO_TRAINING"), None),
    "T_SIG_ROUND": (_sig("training", 1), ("OK", "T_SIG_ROUND", "S_NO_TRAINING"), None),
    "T_ROUND_STALE": (_round_all, ("OK", "T_ROUND_STALE", "S_NO_TRAINING"), "round"),
    "T_SIG_TAU": (_sig("training", 5), ("OK", "T_SIG_TAU", "S_NO_TRAINING"), None),
    "T_ROOT_G_GRADIENT": (_gradient, ("OK", "T_ROOT_G_GRADIENT", "S_NO_TRAINING"), None),
    "T_ROOT_W_MODEL": (_model, ("OK", "T_ROOT_W_MODEL", "S_NO_TRAINING"), "model"),
    "T_PROOF": (_bad_proof("training"), ("OK", "T_PROOF", "S_NO_TRAINING"), None),
    "S_MISSING": (_drop("secagg"), ("OK", "OK", "S_MISSING"), None),
    "S_BIND_ROOT_G": (_claim("secagg", "root_G", 3), ("OK", "OK", "S_BIND_ROOT_G"), None),
    "S_BIND_ROOT_D": (_claim("secagg", "root_D", 2), ("OK", "OK", "S_BIND_ROOT_D"), None),
    "S_BIND_ROOT_W": (_claim("secagg", "root_W", 4), ("OK", "OK", "S_BIND_ROOT_W"), None),
    "S_SIG_CLIENT_ID": (_sig("secagg", 0), ("OK", "OK", "S_SIG_CLIENT_ID"), None),
    "S_SIG_ROUND": (_sig("secagg", 1), ("OK", "OK", "S_SIG_ROUND"), None),
    "S_ROUND_STALE": (_round_secagg, ("OK", "OK", "S_ROUND_STALE"), "round"),
    "S_SIG_ROOT_D": (_sig("secagg", 2), ("OK", "OK", "S_SIG_ROOT_D"), None),
    "S_SIG_ROOT_G": (_sig("secagg", 3), ("OK", "OK", "S_SIG_ROOT_G"), None),
    "S_SIG_ROOT_W": (_sig("secagg", 4), ("OK", "OK", "S_SIG_ROOT_W"), None),
    "S_SIG_ROOT_K": (_sig("secagg", 5), ("OK", "OK", "S_SIG_ROOT_K"), None),
    "S_SIG_TAU": (_sig("secagg", 6), ("OK", "OK", "S_SIG_TAU"), None),
    "S_SIG_MASKED": (_masked_last, ("OK", "OK", "S_SIG_MASKED"), None),
    "S_SIG_PEERS": (_peers, ("OK", "OK", "S_SIG_PEERS"), "peers"),
    "S_PROOF": (_bad_proof("secagg"), ("OK", "OK", "S_PROOF"), None),
}
# S_NO_TRAINING and T_NO_BALANCE are the cascades of the entries above; every other code has its own
STATIC_TAMPERS = [k for k in TAMPERS if not k.endswith("_PROOF")]


def clone(rnd):
    """A copy whose packages, peers and weights can be edited (key handles are shared, not copied)."""
    out = dict(rnd)
    for k in ("clients", "weights", "peers", "balance", "training", "secagg"):
        if k in rnd:
            out[k] = copy.deepcopy(rnd[k])
    return out


def apply(rnd, name, cid):
    """The tamper, in place."""
    TAMPERS[name][0](rnd, cid)


def tampered(rnd, name, cid):
    out = clone(rnd)
    apply(out, name, cid)
    return out


def expected(name):
    return tuple(C[x] for x in TAMPERS[name][1])
