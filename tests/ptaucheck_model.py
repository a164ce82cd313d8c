"""The ptau check on the CPU: an independent restatement of `powersoftau check` over oracle/bn254.py.

Is a .ptau a well-formed Powers of Tau for some tau, alpha and beta, with sections 12-15 the Lagrange
form of sections 2-5?  The model reads the file's bytes itself (iden3 binfile sections, Montgomery
affine points); it shares no code with zkfl/ptaucheck.py or csrc/ptaucheck.hip.  n = 2^power, T, U,
A, B = sections 2-5, b2 = section 6; rnd = z | gamma[power + 2] | rho[2n - 1]; S0(X) = sum_{i < len-1}
rho_i X[i], S1(X) = sum_{i < len-1} rho_i X[i+1]:

  STRUCTURE   T[0] == G1, U[0] == G2; T[1], A[0], B[0], b2 not infinity
  POINTS      every point of sections 2-6, 12-15 all-zero or canonical and on its curve; G2 of order r
  TAU_G1      e(S0(T), U[1]) == e(S1(T), G2)          TAU_G2   e(T[1], S0(U)) == e(G1, S1(U))
  ALPHA_G1    e(S0(A), U[1]) == e(S1(A), G2)          BETA_G1  e(S0(B), U[1]) == e(S1(B), G2)
  BETA_G2     e(B[0], G2) == e(G1, b2)
  L_TAU_G1 | L_TAU_G2 | L_ALPHA_G1 | L_BETA_G1   (12 vs 2, 13 vs 3, 14 vs 4, 15 vs 5)
              sum_p lam_p Lag[p] == sum_i s_i X[i], where position p lies in level k = bitlength(p+1) - 1
              at j = p + 1 - 2^k and
                lam_p = gamma_k w_k^j (z^(2^k) - 1) / (2^k (z - w_k^j))
                s_i   = sum_{k : i < 2^k} gamma_k z^((2^k - i) mod 2^k) / 2^k
              with the levels 0 .. power + 1 for section 12 and 0 .. power for the others.

s_i is written here as the sum the identity gives (block k of a Lagrange section is (1/n_k) sum_i
w_k^(-ij) X[i], and sum_j L_j(z) w_k^(-ij) = z^((n_k - i) mod n_k)); the library computes it as
z^-i times a suffix sum, which is the same number for i >= 1.

A check whose section has a bad point is "not run": the chain checks need their own section and
section 3 (U[1]); BETA_G2 needs sections 5 and 6; a Lagrange check needs both of its sections.  An
unprepared file has no Lagrange checks ("not run", prepared = False).
tests/ptaucheck_tampers.py holds the table this model must satisfy (tests/test_ptaucheck_cpu.py);
tests/test_gpu_ptaucheck.py compares the GPU's outcome with it.
"""
import functools
import struct

from oracle import bn254 as bn

CHECKS = ("STRUCTURE", "POINTS", "TAU_G1", "TAU_G2", "ALPHA_G1", "BETA_G1", "BETA_G2",
          "L_TAU_G1", "L_TAU_G2", "L_ALPHA_G1", "L_BETA_G1")
Q, R = bn.Q, bn.R
G2_SECTIONS = (3, 6, 13)


def sections(buf):
    assert bytes(buf[:4]) == b"ptau"
    nsec = struct.unpack_from("<I", buf, 8)[0]
    off, secs = 12, {}
    for _ in range(nsec):
        typ, size = struct.unpack_from("<IQ", buf, off)
        secs.setdefault(typ, bytes(buf[off + 12:off + 12 + size]))
        off += 12 + size
    return secs


def rnd_split(rnd: bytes, power: int):
    """z | gamma[power + 2] | rho[2n - 1] (32 B little endian each) -> (z, gamma, rho) as ints"""
    v = [int.from_bytes(rnd[i:i + 32], "little") for i in range(0, len(rnd), 32)]
    assert len(v) == 1 + power + 2 + (2 << power) - 1
    return v[0], tuple(v[1:power + 3]), tuple(v[power + 3:])


def _times_r(P):
    """[r]P by hand (bn.mul reduces its scalar mod r)."""
    acc, base, k = None, bn.to_jac(P), R
    while k:
        if k & 1:
            acc = bn.jadd(acc, base)
        base = bn.jdouble(base)
        k >>= 1
    return bn.from_jac(acc)


@functools.lru_cache(maxsize=1 << 16)
def decode(raw: bytes, g2: bool):
    """One stored point -> (ok, point or None)."""
    v = [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]
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


@functools.lru_cache(maxsize=512)
def decode_all(raw: bytes, g2: bool):
    size = 128 if g2 else 64
    out = [decode(raw[i:i + size], g2) for i in range(0, len(raw), size)]
    return tuple(p for _, p in out), tuple(i for i, (ok, _) in enumerate(out) if not ok)


@functools.lru_cache(maxsize=512)
def _msm(raw: bytes, g2: bool, scalars: tuple):
    pts, bad = decode_all(raw, g2)
    assert not bad and len(pts) == len(scalars)
    keep = [(p, s) for p, s in zip(pts, scalars) if p is not None and s]
    return bn.msm([p for p, _ in keep], [s for _, s in keep]) if keep else None


@functools.lru_cache(maxsize=1024)
def _pair_eq_bytes(a1, a2, b1, b2):
    def g1(b):
        return bn.g1_from_bytes_std(b) if any(b) else None

    def g2(b):
        return bn.g2_from_bytes_std(b) if any(b) else None
    B1 = g1(b1)
    return bn.pairing_product([(g1(a1), g2(a2)), (bn.neg(B1) if B1 is not None else None, g2(b2))]) == bn.Fq12.one()


def _pair_eq(A1, A2, B1, B2):
    """e(A1, A2) == e(B1, B2), infinity on either side of a pairing giving 1; memoised on the points"""
    def s1(P):
        return bn.g1_to_bytes_std(P) if P is not None else bytes(64)

    def s2(P):
        return bn.g2_to_bytes_std(P) if P is not None else bytes(128)
    return _pair_eq_bytes(s1(A1), s2(A2), s1(B1), s2(B2))


@functools.lru_cache(maxsize=64)
def lagrange_scalars(power: int, top: int, z: int, gamma: tuple):
    """(lam over the (2 << top) - 1 positions, s over the (1 << top) indices) for the levels 0..top"""
    lam = []
    s = [0] * (1 << top)
    for k in range(top + 1):
        nk = 1 << k
        ninv = pow(nk, R - 2, R)
        w = bn.FR_W[k]
        znk = pow(z, nk, R)
        for j in range(nk):
            wj = pow(w, j, R)
            lam.append(gamma[k] * wj % R * (znk - 1) % R * pow(nk * (z - wj) % R, R - 2, R) % R)
        for i in range(nk):
            s[i] = (s[i] + gamma[k] * pow(z, (nk - i) % nk, R) % R * ninv) % R
    return tuple(lam), tuple(s)


def check(buf, rnd: bytes):
    """-> {"checks": {name: "pass" | "fail" | "not run"}, "status": [0 | 1 | 2 in CHECKS' order],
    "point": (section, index, count) | None, "prepared": bool, "first_failed": name | None}"""
    secs = sections(buf)
    hdr = secs[1]
    assert struct.unpack_from("<I", hdr, 0)[0] == 32 and int.from_bytes(hdr[4:36], "little") == Q
    power = struct.unpack_from("<I", hdr, 36)[0]
    n = 1 << power
    prepared = all(t in secs for t in (12, 13, 14, 15))
    z, gamma, rho = rnd_split(rnd, power)
    assert z and pow(z, 2 * n, R) != 1 and all(x < R for x in (z,) + gamma + rho)
    st = {k: "pass" for k in CHECKS}

    # points, in file order
    order = (2, 3, 4, 5, 6) + ((12, 13, 14, 15) if prepared else ())
    pts, bad, point = {}, {}, None
    for t in order:
        pts[t], bad[t] = decode_all(secs[t], t in G2_SECTIONS)
        if bad[t] and point is None:
            point = (t, bad[t][0], len(bad[t]))
    if point:
        st["POINTS"] = "fail"
    T, U, A, B = secs[2], secs[3], secs[4], secs[5]

    # structure
    g1 = bn.g1_to_bytes_mont(bn.G1_GEN)
    g2 = bn.g2_to_bytes_mont(bn.G2_GEN)
    if not (T[:64] == g1 and U[:128] == g2 and any(T[64:128]) and any(A[:64]) and any(B[:64]) and any(secs[6])):
        st["STRUCTURE"] = "fail"

    def verdict(name, ran, holds):
        st[name] = "not run" if not ran else ("pass" if holds() else "fail")

    def chain(t, g2s=False):
        """(S0, S1) of section t"""
        cnt = len(pts[t])
        s0 = tuple(rho[:cnt - 1]) + (0,)
        s1 = (0,) + tuple(rho[:cnt - 1])
        return _msm(secs[t], g2s, s0), _msm(secs[t], g2s, s1)

    def g1_chain(t):
        S0, S1 = chain(t)
        return _pair_eq(S0, pts[3][1], S1, bn.G2_GEN)

    def g2_chain():
        S0, S1 = chain(3, True)
        return _pair_eq(pts[2][1], S0, bn.G1_GEN, S1)
    ok = {t: not bad[t] for t in order}
    verdict("TAU_G1", ok[2] and ok[3], lambda: g1_chain(2))
    verdict("TAU_G2", ok[2] and ok[3], g2_chain)
    verdict("ALPHA_G1", ok[4] and ok[3], lambda: g1_chain(4))
    verdict("BETA_G1", ok[5] and ok[3], lambda: g1_chain(5))
    verdict("BETA_G2", ok[5] and ok[6], lambda: _pair_eq(pts[5][0], bn.G2_GEN, bn.G1_GEN, pts[6][0]))

    def lagrange(src, dst):
        g2s = src == 3
        top = power + 1 if src == 2 else power
        lam, s = lagrange_scalars(power, top, z, gamma)
        assert len(lam) == len(pts[dst])
        return _msm(secs[dst], g2s, lam) == _msm(secs[src], g2s, s[:len(pts[src])])
    for name, src, dst in (("L_TAU_G1", 2, 12), ("L_TAU_G2", 3, 13), ("L_ALPHA_G1", 4, 14), ("L_BETA_G1", 5, 15)):
        verdict(name, prepared and ok[src] and ok[dst], lambda: lagrange(src, dst))
    failed = [k for k in CHECKS if st[k] == "fail"]
    return dict(checks=st, status=[("pass", "fail", "not run").index(st[k]) for k in CHECKS], point=point,
                prepared=prepared, first_failed=failed[0] if failed else None)
