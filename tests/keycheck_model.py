"""The key check on the CPU: an independent restatement of `zkey check` over oracle/bn254.py.

Is a .zkey the Groth16 proving key of a constraint system over a prepared .ptau, for some delta and
gamma?  The model reads the two files' bytes itself (iden3 binfile sections, Montgomery affine
points) and takes the system as the builder's ``cons`` ([(A, B, C)] of {wire: coefficient}); it
shares no code with zkfl/keycheck.py or csrc/keycheck.hip.  With rho over the wires and sigma over
the domain, a(v), b(v), c(v) the rows evaluated on v (plus the public rows a[m + s] += v[s]) and
K(v) = MSM(Lb, a(v)) + MSM(La, b(v)) + MSM(L, c(v)):

  header        counts, q, r; alpha1, beta1, beta2 are the ptau's; gamma2, delta1, delta2 proper
                points; e(delta1, G2) == e(G1, delta2)
  points        every point all-zero or canonical and on its curve; G2 points of order r
  coefficients  section 4 on rho == a(rho), b(rho) row for row
  A, B1, B2     MSM(section 5 | 6 | 7, rho) == MSM(L, a) | MSM(L, b) | MSM(L2, b)
  IC            e(MSM(section 3, rho_pub), gamma2) == e(K(rho_pub), G2)
  C             e(MSM(section 8, rho_prv), delta2) == e(K(rho_prv), G2)
  H             e(MSM(section 9, sigma), delta2) == e(MSM(H0, sigma), G2)

A section with a bad point (and IC / C / H under an unusable gamma2 / delta2) is "not run".
tests/test_keycheck_cpu.py holds the tamper table this model must satisfy; tests/test_gpu_keycheck.py
compares the GPU's outcome with it.
"""
import functools
import struct

from oracle import bn254 as bn

CHECKS = ("header", "points", "coefficients", "A", "B1", "B2", "IC", "C", "H")
Q, R = bn.Q, bn.R
_R2_INV = pow(pow(2, 512, R), R - 2, R)   # section 4 stores coef * 2^512 mod r


def sections(buf, magic):
    assert bytes(buf[:4]) == magic
    nsec = struct.unpack_from("<I", buf, 8)[0]
    off, secs = 12, {}
    for _ in range(nsec):
        typ, size = struct.unpack_from("<IQ", buf, off)
        secs.setdefault(typ, bytes(buf[off + 12:off + 12 + size]))
        off += 12 + size
    return secs


def _ints(b):
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def _times_r(P):
    """[r]P by hand (bn.mul reduces its scalar mod r)."""
    acc, base, k = None, bn.to_jac(P), R
    while k:
        if k & 1:
            acc = bn.jadd(acc, base)
        base = bn.jdouble(base)
        k >>= 1
    return bn.from_jac(acc)


def decode(raw, g2):
    """One stored point -> (ok, point or None).  ok: all-zero, or canonical coordinates on the
    curve (G2: and of order r)."""
    v = _ints(raw)
    if not any(v):
        return True, None
    if any(x >= Q for x in v):
        return False, None
    v = [bn.from_mont(x, Q) for x in v]
    P = (bn.Fq2(v[0], v[1]), bn.Fq2(v[2], v[3])) if g2 else (v[0], v[1])
    if not bn.on_curve(P):
        return False, None
    if g2 and _times_r(P) is not None:
        return False, None
    return True, P


def decode_all(raw, g2):
    size = 128 if g2 else 64
    out = [decode(raw[i:i + size], g2) for i in range(0, len(raw), size)]
    bad = [i for i, (ok, _) in enumerate(out) if not ok]
    return [p for _, p in out], bad


def rows(cons, n_public, n, v):
    """a(v), b(v), c(v) on the domain."""
    a, b, c = [0] * n, [0] * n, [0] * n
    for j, (A, B, C) in enumerate(cons):
        a[j] = sum(k * v[w] for w, k in A.items()) % R
        b[j] = sum(k * v[w] for w, k in B.items()) % R
        c[j] = sum(k * v[w] for w, k in C.items()) % R
    for s in range(n_public + 1):
        a[len(cons) + s] = (a[len(cons) + s] + v[s]) % R
    return a, b, c


def _freeze(cons):
    return tuple(tuple(tuple(sorted(m.items())) for m in con) for con in cons)


@functools.lru_cache(maxsize=16)
def _ptau_side(ptau_buf, frozen, n_wires, n_public, n, rho, sigma):
    """Everything that depends on the ptau and the system alone (shared among the keys a test
    checks against them): the blocks' points and the right-hand sides."""
    cons = [tuple(dict(m) for m in con) for con in frozen]
    power = n.bit_length() - 1
    ps = sections(ptau_buf, b"ptau")

    def block(t, p, g2=False):
        size = 128 if g2 else 64
        raw = ps[t][((1 << p) - 1) * size:((2 << p) - 1) * size]
        pts = [bn.g2_from_bytes_mont(raw[i:i + size]) if g2 else bn.g1_from_bytes_mont(raw[i:i + size])
               for i in range(0, len(raw), size)]
        assert len(pts) == 1 << p
        return pts
    L, L2, La, Lb = block(12, power), block(13, power, True), block(14, power), block(15, power)
    H0 = block(12, power + 1)[1::2]
    pub = [x if w <= n_public else 0 for w, x in enumerate(rho)]
    prv = [0 if w <= n_public else x for w, x in enumerate(rho)]
    a, b, _ = rows(cons, n_public, n, rho)

    def K(v):
        av, bv, cv = rows(cons, n_public, n, v)
        return bn.add(bn.add(bn.msm(Lb, av), bn.msm(La, bv)), bn.msm(L, cv))
    return dict(a=a, b=b, La=bn.msm(L, a), Lb=bn.msm(L, b), L2b=bn.msm(L2, b), Kpub=K(pub), Kprv=K(prv),
                H0=bn.msm(H0, list(sigma)), alpha1=ps[4][:64], beta1=ps[5][:64], beta2=ps[6][:128])


@functools.lru_cache(maxsize=256)
def _pair_eq_bytes(p, q2, kp, k2):
    return bn.pairing_product([(bn.g1_from_bytes_std(p), bn.g2_from_bytes_std(q2)),
                               (bn.neg(bn.g1_from_bytes_std(kp)), bn.g2_from_bytes_std(k2))]) == bn.Fq12.one()


def _pair_eq(P, Q2, Kp, K2=bn.G2_GEN):
    """e(P, Q2) == e(Kp, K2); memoised on the points (most tampers leave most pairings as they were)"""
    return _pair_eq_bytes(bn.g1_to_bytes_std(P), bn.g2_to_bytes_std(Q2), bn.g1_to_bytes_std(Kp), bn.g2_to_bytes_std(K2))


def check(cons, n_wires, n_public, ptau_buf, zkey_buf, rho, sigma):
    """-> {"checks": {name: "pass" | "fail" | "not run"}, "point": (section, index, count) | None,
    "coef": (matrix, row, count) | None, "first_failed": name | None}"""
    zs = sections(zkey_buf, b"zkey")
    hdr = zs[2]
    n8q, = struct.unpack_from("<I", hdr, 0)
    q = int.from_bytes(hdr[4:36], "little")
    n8r, = struct.unpack_from("<I", hdr, 36)
    r = int.from_bytes(hdr[40:72], "little")
    nv, npub, n = struct.unpack_from("<III", hdr, 72)
    want_n = 1
    while want_n < len(cons) + n_public + 1:
        want_n *= 2
    st = {k: "pass" for k in CHECKS}
    counts_ok = (n8q, q, n8r, r, nv, npub, n) == (32, Q, 32, R, n_wires, n_public, want_n)
    if not counts_ok:   # nothing below is defined for other counts
        st = {k: "not run" for k in CHECKS}
        st["header"] = "fail"
        return dict(checks=st, point=None, coef=None, first_failed="header")
    side = _ptau_side(bytes(ptau_buf), _freeze(cons), n_wires, n_public, n, tuple(rho), tuple(sigma))
    raw = dict(alpha1=hdr[84:148], beta1=hdr[148:212], beta2=hdr[212:340], gamma2=hdr[340:468],
               delta1=hdr[468:532], delta2=hdr[532:660])
    order = ("alpha1", "beta1", "beta2", "gamma2", "delta1", "delta2")
    hp = {k: decode(raw[k], k.endswith("2")) for k in order}
    usable = {k: hp[k][0] and hp[k][1] is not None for k in order}

    # points
    point = None
    hdr_bad = [i for i, k in enumerate(order) if not hp[k][0]]
    if hdr_bad:
        point = (2, hdr_bad[0], len(hdr_bad))
    pts, bad = {}, {}
    for t in (3, 5, 6, 7, 8, 9):
        pts[t], bad[t] = decode_all(zs[t], t == 7)
        if bad[t] and point is None:
            point = (t, bad[t][0], len(bad[t]))
    if point:
        st["points"] = "fail"

    # header
    ok = raw["alpha1"] == side["alpha1"] and raw["beta1"] == side["beta1"] and raw["beta2"] == side["beta2"]
    ok = ok and usable["gamma2"] and usable["delta1"] and usable["delta2"]
    if ok:
        ok = _pair_eq(hp["delta1"][1], bn.G2_GEN, bn.G1_GEN, hp["delta2"][1])
    if not ok:
        st["header"] = "fail"

    # coefficients: section 4 as linear maps on rho
    ncoef, = struct.unpack_from("<I", zs[4], 0)
    got = [[0] * n, [0] * n]
    for i in range(ncoef):
        m, c, s = struct.unpack_from("<III", zs[4], 4 + 44 * i)
        val = int.from_bytes(zs[4][16 + 44 * i:48 + 44 * i], "little") * _R2_INV % R
        got[m][c] = (got[m][c] + val * rho[s]) % R
    diff = [(m, j) for m, want in ((0, side["a"]), (1, side["b"])) for j in range(n) if got[m][j] != want[j]]
    coef = None
    if diff:
        st["coefficients"] = "fail"
        coef = (diff[0][0], diff[0][1], len(diff))

    rho_pub, rho_prv = list(rho[:n_public + 1]), list(rho[n_public + 1:])

    def verdict(name, ran, holds):
        st[name] = "not run" if not ran else ("pass" if holds() else "fail")
    verdict("A", not bad[5], lambda: bn.msm(pts[5], list(rho)) == side["La"])
    verdict("B1", not bad[6], lambda: bn.msm(pts[6], list(rho)) == side["Lb"])
    verdict("B2", not bad[7], lambda: bn.msm(pts[7], list(rho)) == side["L2b"])
    verdict("IC", not bad[3] and usable["gamma2"],
            lambda: _pair_eq(bn.msm(pts[3], rho_pub), hp["gamma2"][1], side["Kpub"]))
    verdict("C", not bad[8] and usable["delta2"],
            lambda: _pair_eq(bn.msm(pts[8], rho_prv), hp["delta2"][1], side["Kprv"]))
    verdict("H", not bad[9] and usable["delta2"],
            lambda: _pair_eq(bn.msm(pts[9], list(sigma)), hp["delta2"][1], side["H0"]))
    failed = [k for k in CHECKS if st[k] == "fail"]
    return dict(checks=st, point=point, coef=coef, first_failed=failed[0] if failed else None)
