"""Plain-Python model of round preparation (zkfl_round_prepare, zkfl/prepare.py).

Built from zkfl/clients.py's functions -- vector_hash, merkle_tree, merkle_proof, gradient_commitment,
pairwise_mask -- which restate the reference's client (tests/full_system_simulation.mjs:139-238,
:308-335, :411-438, :511-553, :558-637), plus what clients.py does not take: the batch rows
(`batch_idx`) and explicit peers and keys.  A spec is zkfl/prepare.py's.  Per phase the model gives the
input.json dict and, through wprog.input_bytes(circuits.build(...), input_json), the flattened input
vector the device must reproduce byte for byte.
"""
import numpy as np

from zkfl import circuits, clients, wprog
from zkfl.field import R, poseidon_hash

OK, NORM = 0, 1


def shapes(spec, peers=None):
    """{phase: circuit shape} of a spec."""
    S, dim, depth, batch, prec = (int(spec[k]) for k in ("samples", "dim", "depth", "batch", "precision"))
    np_ = len(spec["peers"][0]) if spec.get("peers") else 0
    out = {"balance": ("balance_unified", S, depth, dim), "training": ("sgd_verified", batch, dim, depth, prec)}
    if np_:
        out["secagg"] = ("secure_masked_update", dim, np_)
    return out


def gradient(features, labels, rows, weights, precision):
    """_computeVerifiedGradient (:511-553) over the chosen rows: Python's // is Math.floor."""
    dim, div = len(weights), len(rows) * precision
    summed = [0] * dim
    for r in rows:
        pred = sum(features[r][j] * weights[j] for j in range(dim))
        err = pred - labels[r] * precision
        for j in range(dim):
            summed[j] += err * features[r][j]
    grad = [s // div for s in summed]
    rem = [s - q * div for s, q in zip(summed, grad)]
    assert all(0 <= x < div for x in rem)
    return grad, summed, rem


def client(spec, i):
    """Client i of a spec -> {"balance", "training", "secagg" (with peers): input.json dicts, "gradient",
    "roots" (D, G, W, K), "masked", "c1", "norm", "status"}."""
    cid = int(spec["ids"][i])
    S, dim, depth, batch, prec = (int(spec[k]) for k in ("samples", "dim", "depth", "batch", "precision"))
    feats = [[int(x) for x in row] for row in spec["features"][i]]
    labels = [int(x) for x in spec["labels"][i]]
    weights = [int(w) for w in spec["weights"]]
    rnd, tau = int(spec["round"]), int(spec["tau_squared"])
    rows = [int(x) for x in spec["batch_idx"][i]] if spec.get("batch_idx") is not None else list(range(batch))
    tree = clients.merkle_tree([clients.vector_hash(feats[s] + [labels[s]]) for s in range(S)], depth)
    root_D = tree.root

    def openings(idx):
        sib, pth = zip(*[clients.merkle_proof(tree, r, depth) for r in idx])
        return [[str(s) for s in row] for row in sib], [[str(p) for p in row] for row in pth]

    c1 = sum(labels)
    sib, pth = openings(range(S))
    balance = {"client_id": str(cid), "root": str(root_D), "N_public": str(S), "c0": str(S - c1), "c1": str(c1),
               "features": [[str(x) for x in row] for row in feats], "labels": [str(x) for x in labels],
               "siblings": sib, "pathIndices": pth}

    grad, summed, rem = gradient(feats, labels, rows, weights, prec)
    g_field = [g % R for g in grad]
    root_W = clients.vector_hash(weights)
    root_G = clients.gradient_commitment(g_field, cid, rnd)
    sib, pth = openings(rows)
    training = {"client_id": str(cid), "round": str(rnd), "root_D": str(root_D), "root_G": str(root_G),
                "root_W": str(root_W), "tauSquared": str(tau), "weights": [str(w) for w in weights],
                "expectedSummedGrad": [str(s) for s in summed], "remainder": [str(x) for x in rem],
                "gradPos": [str(g if g >= 0 else 0) for g in grad], "gradNeg": [str(-g if g < 0 else 0) for g in grad],
                "features": [[str(x) for x in feats[r]] for r in rows], "labels": [str(labels[r]) for r in rows],
                "siblings": sib, "pathIndices": pth}
    norm = sum(g * g for g in grad)
    out = {"balance": balance, "training": training, "gradient": grad, "c1": c1, "norm": norm,
           "status": NORM if norm > tau else OK, "roots": [root_D, root_G, root_W, 0], "masked": None}
    if spec.get("peers"):
        peers = [int(p) for p in spec["peers"][i]]
        keys = [int(k) for k in spec["keys"][i]]
        master = int(spec["master_keys"][i])
        root_K = poseidon_hash([master] + keys)
        masked = list(g_field)
        for p, k in zip(peers, keys):
            m = clients.pairwise_mask(k, rnd, cid, p, dim)
            sign = 1 if cid < p else -1
            masked = [(a + sign * b) % R for a, b in zip(masked, m)]
        out["secagg"] = {"client_id": str(cid), "round": str(rnd), "root_D": str(root_D), "root_G": str(root_G),
                         "root_W": str(root_W), "root_K": str(root_K), "tauSquared": str(tau),
                         "masked_update": [str(x) for x in masked], "peer_ids": [str(p) for p in peers],
                         "gradient": [str(g) for g in g_field], "master_key": str(master),
                         "shared_keys": [str(k) for k in keys]}
        out["roots"][3] = root_K
        out["masked"] = masked
    return out


def _frs(values) -> np.ndarray:
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint8).reshape(-1, 32)


def result(spec, per_client=None) -> dict:
    """The arrays Context.round_prepare returns, from the model (per_client: [client(spec, i)] when the
    caller has them already)."""
    n = len(spec["ids"])
    cl = per_client if per_client is not None else [client(spec, i) for i in range(n)]
    sh = shapes(spec)
    res = {}
    for phase, shape in sh.items():
        b = circuits.build(*shape)
        res[f"{phase}_inputs"] = np.stack([np.frombuffer(wprog.input_bytes(b, c[phase]), dtype=np.uint8).reshape(-1, 32)
                                           for c in cl])
    res["roots"] = np.stack([_frs(c["roots"]) for c in cl])
    res["gradients"] = np.array([c["gradient"] for c in cl], dtype=np.int64)
    if "secagg" in sh:
        res["masked"] = np.stack([_frs(c["masked"]) for c in cl])
    res["c1"] = np.array([c["c1"] for c in cl], dtype=np.uint32)
    res["status"] = np.array([c["status"] for c in cl], dtype=np.uint32)
    return res


def harness_spec(ids, samples, dim, depth, batch, precision=1000, tau_squared=100000000, rnd=1, weights=None,
                 peers=True, group_size=None, seed=None):
    """The harness's defaults as a spec: clients.Client's dataset under JsLcg(12345 + id) (or the one
    seed for every client), weights 0, every client's peers the others of its group."""
    from zkfl import prepare
    ids = [int(c) for c in ids]
    data = [prepare.harness_dataset(c, samples, dim, seed) for c in ids]
    spec = {"ids": ids, "samples": samples, "dim": dim, "depth": depth, "batch": batch, "precision": precision,
            "features": [f for f, _ in data], "labels": [l for _, l in data],
            "weights": list(weights) if weights is not None else [0] * dim, "round": rnd, "tau_squared": tau_squared}
    if peers and len(ids) > 1:
        spec["peers"], spec["keys"], spec["master_keys"] = prepare.harness_keys(ids, group_size)
    return spec
