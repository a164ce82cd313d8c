"""Model of the combined round check (zkfl_groth16_verify_round), on oracle/pairing_tower.py only.

A job is (A, B, X, C, k): pi_a, pi_b (bn254 G2 affine or None), vk_x, pi_c and the index of its
key; a key is (alpha1, beta2, gamma2, delta2).  Points are oracle.bn254 affine points, None =
infinity.  The expected value of a round is the product of the per-job check values raised to
their z_i:

    prod_i ( final_exp(miller_loop([(-A_i, B_i), (alpha, beta), (X_i, gamma), (C_i, delta)])) )^{z_i}

(a pair with an infinite point contributes 1, as miller_loop skips it).  `sums_first` is the
formula the GPU evaluates: one pair per job, three per key, one final exponentiation.  Screened
jobs are the caller's to leave out.  Check values are cached per distinct (key, public, proof).
"""
from oracle import bn254 as bn
from oracle import pairing_tower as T

GT_ONE = T.gt_bytes(T.F12_ONE)


def f12_pow(x, e):
    r = T.F12_ONE
    for bit in bin(e)[2:] if e else "":
        r = T.f12_sqr(r)
        if bit == "1":
            r = T.f12_mul(r, x)
    return r


def check_value(A, B, X, C, key):
    alpha, beta, gamma, delta = key
    g2 = T.from_bn254_g2
    return T.final_exp(T.miller_loop([(bn.neg(A), g2(B)), (alpha, g2(beta)), (X, g2(gamma)), (C, g2(delta))]))


def product_of_powers(values, zs):
    """values: the jobs' check values (check_value / job_value) -> the round's GT element."""
    f = T.F12_ONE
    for v, z in zip(values, zs):
        f = T.f12_mul(f, f12_pow(v, z))
    return f


def sums_first(jobs, keys, zs):
    g2 = T.from_bn254_g2
    pairs = [(bn.mul(bn.neg(A), z) if A is not None else None, g2(B)) for (A, B, _, _, _), z in zip(jobs, zs)]
    for k, (alpha, beta, gamma, delta) in enumerate(keys):
        mine = [(j, z) for j, z in zip(jobs, zs) if j[4] == k]
        if not mine:
            continue
        Z = sum(z for _, z in mine) % bn.R
        X = C = None
        for (_, _, Xi, Ci, _), z in mine:
            X = bn.add(X, bn.mul(Xi, z))
            C = bn.add(C, bn.mul(Ci, z))
        pairs += [(bn.mul(alpha, Z), g2(beta)), (X, g2(gamma)), (C, g2(delta))]
    return T.final_exp(T.miller_loop(pairs))


_CACHE = {}


def job_value(vk, key_id, pub, proof):
    """vk: oracle.groth16.parse_zkey's dict (alpha1, beta2, gamma2, delta2, IC); pub: ints < r;
    proof: 256 B with canonical coordinates -> the job's check value (cached)."""
    tag = (key_id, tuple(pub), bytes(proof))
    if tag not in _CACHE:
        assert len(pub) == len(vk["IC"]) - 1 and all(0 <= x < bn.R for x in pub)
        X = vk["IC"][0]
        for x, P in zip(pub, vk["IC"][1:]):
            X = bn.add(X, bn.mul(P, int(x)))
        A, B, C = bn.g1_from_bytes_std(proof[:64]), bn.g2_from_bytes_std(proof[64:192]), bn.g1_from_bytes_std(proof[192:])
        _CACHE[tag] = check_value(A, B, X, C, (vk["alpha1"], vk["beta2"], vk["gamma2"], vk["delta2"]))
    return _CACHE[tag]


def expected_gt(jobs, zs) -> bytes:
    """jobs: [(vk, key_id, pub ints, proof bytes)], none of them screened -> 384 B."""
    # equal jobs share a value: v^z1 v^z2 = v^(z1 + z2), so a replicated round costs one power per distinct job
    exps, values = {}, {}
    for j, z in zip(jobs, zs):
        v = job_value(*j)
        exps[id(v)] = exps.get(id(v), 0) + z
        values[id(v)] = v
    return T.gt_bytes(product_of_powers([values[t] for t in exps], [exps[t] for t in exps]))
