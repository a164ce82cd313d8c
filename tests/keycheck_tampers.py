"""Tampered proving keys for the key check's tests: byte-level edits of a .zkey, with the checks each
must fail and the checks it must leave "not run".  The table is the contract both the CPU model
(tests/test_keycheck_cpu.py) and the GPU check (tests/test_gpu_keycheck.py) are held to; every check
has a tamper that only it catches, so no check is vacuous.  Point arithmetic is oracle/bn254.py's.
"""
import struct

from oracle import bn254 as bn

Q, R = bn.Q, bn.R
HDR = dict(alpha1=(84, 64), beta1=(148, 64), beta2=(212, 128), gamma2=(340, 128), delta1=(468, 64), delta2=(532, 128))


def zsecs(buf):
    nsec = struct.unpack_from("<I", buf, 8)[0]
    off, secs = 12, {}
    for _ in range(nsec):
        typ, size = struct.unpack_from("<IQ", buf, off)
        secs.setdefault(typ, (off + 12, size))
        off += 12 + size
    return secs


def patch(buf, off, data):
    return bytes(buf[:off]) + bytes(data) + bytes(buf[off + len(data):])


def _size(t):
    return 128 if t == 7 else 64


def raw_point(buf, t, i):
    o = zsecs(buf)[t][0] + i * _size(t)
    return bytes(buf[o:o + _size(t)])


def count(buf, t):
    return zsecs(buf)[t][1] // _size(t)


def put_raw(buf, t, i, raw):
    return patch(buf, zsecs(buf)[t][0] + i * _size(t), raw)


def get_point(buf, t, i):
    raw = raw_point(buf, t, i)
    return bn.g2_from_bytes_mont(raw) if t == 7 else bn.g1_from_bytes_mont(raw)


def put_point(buf, t, i, P):
    return put_raw(buf, t, i, bn.g2_to_bytes_mont(P) if t == 7 else bn.g1_to_bytes_mont(P))


def live(buf, t):
    """indices of the section's points that are not infinity"""
    return [i for i in range(count(buf, t)) if any(raw_point(buf, t, i))]


def swap(buf, t):
    """two different points of section t exchanged"""
    idx = live(buf, t)
    i = idx[0]
    j = next(k for k in idx[1:] if raw_point(buf, t, k) != raw_point(buf, t, i))
    a, b = raw_point(buf, t, i), raw_point(buf, t, j)
    return put_raw(put_raw(buf, t, i, b), t, j, a)


def scaled(buf, t, k, i=None):
    i = live(buf, t)[0] if i is None else i
    return put_point(buf, t, i, bn.mul(get_point(buf, t, i), k))


def hdr_scaled(buf, name, k):
    o, size = HDR[name]
    o += zsecs(buf)[2][0]
    raw = bytes(buf[o:o + size])
    if size == 128:
        return patch(buf, o, bn.g2_to_bytes_mont(bn.mul(bn.g2_from_bytes_mont(raw), k)))
    return patch(buf, o, bn.g1_to_bytes_mont(bn.mul(bn.g1_from_bytes_mont(raw), k)))


def hdr_raw(buf, name, raw):
    return patch(buf, zsecs(buf)[2][0] + HDR[name][0], raw)


def coef_plus_one(buf, k=0):
    """section 4, entry k: coefficient + 1 (stored as coef * 2^512 mod r)"""
    o = zsecs(buf)[4][0] + 4 + 44 * k + 12
    v = (int.from_bytes(buf[o:o + 32], "little") + pow(2, 512, R)) % R
    return patch(buf, o, v.to_bytes(32, "little"))


def term_moved(buf, k=0):
    """section 4, entry k: the term moves to the next constraint"""
    o = zsecs(buf)[4][0] + 4 + 44 * k
    m, c, s = struct.unpack_from("<III", buf, o)
    return patch(buf, o, struct.pack("<III", m, c + 1, s))


def off_curve(buf, t, i):
    """point i of section t with y + 1 (Montgomery form): canonical, not on the curve (an infinity
    becomes (0, 1), which is on neither curve)"""
    raw = raw_point(buf, t, i)
    yo = 64 if t == 7 else 32
    y = (int.from_bytes(raw[yo:yo + 32], "little") + 1) % Q
    return put_raw(buf, t, i, raw[:yo] + y.to_bytes(32, "little") + raw[yo + 32:])


def plus_q(buf, t, i):
    """point i of section t with x + q: the same point, coordinate not canonical"""
    raw = raw_point(buf, t, i)
    assert any(raw)
    x = int.from_bytes(raw[:32], "little") + Q
    return put_raw(buf, t, i, x.to_bytes(32, "little") + raw[32:])


def _fq2_sqrt(a):
    """a square root in Fq2 = Fq[u]/(u^2 + 1), or None (q = 3 mod 4)"""
    norm = (a.c0 * a.c0 + a.c1 * a.c1) % Q          # a root x0 + x1 u has x0^2 = (a0 +- sqrt(norm)) / 2
    s = pow(norm, (Q + 1) // 4, Q)
    if s * s % Q != norm:
        return None
    for t in (s, -s % Q):
        x0sq = (a.c0 + t) * pow(2, Q - 2, Q) % Q
        x0 = pow(x0sq, (Q + 1) // 4, Q)
        if x0 and x0 * x0 % Q == x0sq:
            root = bn.Fq2(x0, a.c1 * pow(2 * x0, Q - 2, Q) % Q)
            if root * root == a:
                return root
    return None


def twist_point_outside_g2(seed=5):
    """a point of the twist that is not of order r"""
    x = seed
    while True:
        X = bn.Fq2(x, 1)
        Y = _fq2_sqrt(X * X * X + bn.B2)
        if Y is not None:
            P = (X, Y)
            assert bn.on_curve(P)
            acc, base, k = None, bn.to_jac(P), R
            while k:
                if k & 1:
                    acc = bn.jadd(acc, base)
                base = bn.jdouble(base)
                k >>= 1
            if bn.from_jac(acc) is not None:
                return P
        x += 1


# name -> (edit, checks that must fail, checks that must read "not run"); every other check passes
TAMPERS = {
    "A_swapped": (lambda zk: swap(zk, 5), {"A"}, set()),
    "B1_doubled": (lambda zk: scaled(zk, 6, 2), {"B1"}, set()),
    "B2_replaced": (lambda zk: put_point(zk, 7, live(zk, 7)[0], bn.mul(bn.G2_GEN, 12345)), {"B2"}, set()),
    "IC_changed": (lambda zk: put_point(zk, 3, 0, bn.add(get_point(zk, 3, 0), bn.G1_GEN)), {"IC"}, set()),
    "C_scaled": (lambda zk: scaled(zk, 8, 3), {"C"}, set()),
    "H_swapped": (lambda zk: swap(zk, 9), {"H"}, set()),
    "coef_plus_one": (coef_plus_one, {"coefficients"}, set()),
    "term_moved": (term_moved, {"coefficients"}, set()),
    "delta1_scaled": (lambda zk: hdr_scaled(zk, "delta1", 5), {"header"}, set()),
    "alpha1_replaced": (lambda zk: hdr_raw(zk, "alpha1", bn.g1_to_bytes_mont(bn.mul(bn.G1_GEN, 777))), {"header"}, set()),
    # encodings: the section is named by the points check and takes no part in its own check
    "A_off_curve": (lambda zk: off_curve(zk, 5, live(zk, 5)[0]), {"points"}, {"A"}),
    "A_plus_q": (lambda zk: plus_q(zk, 5, live(zk, 5)[0]), {"points"}, {"A"}),
    "B2_outside_g2": (lambda zk: put_point(zk, 7, live(zk, 7)[0], twist_point_outside_g2()), {"points"}, {"B2"}),
    "delta2_infinity": (lambda zk: hdr_raw(zk, "delta2", bytes(128)), {"header"}, {"C", "H"}),
}


def expected(name):
    """-> {check: state} of tamper `name`"""
    _, fails, skipped = TAMPERS[name]
    return {c: "fail" if c in fails else "not run" if c in skipped else "pass"
            for c in ("header", "points", "coefficients", "A", "B1", "B2", "IC", "C", "H")}
