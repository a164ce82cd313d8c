"""Tampered Powers of Tau files for the ptau check's tests: byte-level edits of a .ptau, with the
checks each must fail and the checks it must leave "not run".  The table is the contract both the
CPU model (tests/test_ptaucheck_cpu.py) and the GPU check (tests/test_gpu_ptaucheck.py) are held to;
every check has a tamper that only it catches, so no check is vacuous.  Point arithmetic is
oracle/bn254.py's; replacement points are valid group elements unless the tamper says otherwise.

An edit takes (buf, env): buf a prepared file of power >= 2 with at least one contribution, env.prepare
(an unprepared file -> the prepared one, on whatever backend the test has) and env.other (a prepared
file of the same power with another tau).
"""
import struct

from keycheck_tampers import twist_point_outside_g2
from oracle import bn254 as bn
from oracle import ptau as optau

Q, R = bn.Q, bn.R
CHECKS = ("STRUCTURE", "POINTS", "TAU_G1", "TAU_G2", "ALPHA_G1", "BETA_G1", "BETA_G2",
          "L_TAU_G1", "L_TAU_G2", "L_ALPHA_G1", "L_BETA_G1")
G2_SECTIONS = (3, 6, 13)
CHAIN = {2: "TAU_G1", 3: "TAU_G2", 4: "ALPHA_G1", 5: "BETA_G1"}
LAGRANGE = {12: "L_TAU_G1", 13: "L_TAU_G2", 14: "L_ALPHA_G1", 15: "L_BETA_G1"}
# the checks a section with a bad point takes out ("not run")
GATED = {2: {"TAU_G1", "TAU_G2", "L_TAU_G1"}, 3: {"TAU_G1", "TAU_G2", "ALPHA_G1", "BETA_G1", "L_TAU_G2"},
         4: {"ALPHA_G1", "L_ALPHA_G1"}, 5: {"BETA_G1", "BETA_G2", "L_BETA_G1"}, 6: {"BETA_G2"},
         12: {"L_TAU_G1"}, 13: {"L_TAU_G2"}, 14: {"L_ALPHA_G1"}, 15: {"L_BETA_G1"}}


# ---- files ----
def psecs(buf):
    nsec = struct.unpack_from("<I", buf, 8)[0]
    off, secs = 12, {}
    for _ in range(nsec):
        typ, size = struct.unpack_from("<IQ", buf, off)
        secs.setdefault(typ, (off + 12, size))
        off += 12 + size
    return secs


def binfile(secs: dict) -> bytes:
    out = [b"ptau", struct.pack("<II", 1, len(secs))]
    for t in sorted(secs):
        out += [struct.pack("<IQ", t, len(secs[t])), secs[t]]
    return b"".join(out)


def split(buf) -> dict:
    return {t: bytes(buf[o:o + sz]) for t, (o, sz) in psecs(buf).items()}


def power_of(buf) -> int:
    return struct.unpack_from("<I", buf, psecs(buf)[1][0] + 36)[0]


def unprepared(buf) -> bytes:
    return binfile({t: s for t, s in split(buf).items() if t < 12})


def _size(t):
    return 128 if t in G2_SECTIONS else 64


def _enc(t, P):
    return bn.g2_to_bytes_mont(P) if t in G2_SECTIONS else bn.g1_to_bytes_mont(P)


def _dec(t, raw):
    return bn.g2_from_bytes_mont(raw) if t in G2_SECTIONS else bn.g1_from_bytes_mont(raw)


def _gen(t):
    return bn.G2_GEN if t in G2_SECTIONS else bn.G1_GEN


def build(power, contributions, prepared=True) -> bytes:
    """A .ptau from oracle/ptau.py: `powersoftau new`, then one contribution per (tau, alpha, beta)
    with a 4-byte dummy record each (the check does not read section 7), then `prepare phase2`."""
    n = 1 << power
    secs = {2: [bn.G1_GEN] * (2 * n - 1), 3: [bn.G2_GEN] * n, 4: [bn.G1_GEN] * n, 5: [bn.G1_GEN] * n, 6: bn.G2_GEN}
    for tau, alpha, beta in contributions:
        secs = optau.contribute(secs, power, tau, alpha, beta)
    out = {1: struct.pack("<I", 32) + Q.to_bytes(32, "little") + struct.pack("<II", power, power),
           7: struct.pack("<I", len(contributions)) + bytes(4 * len(contributions))}
    for t in (2, 3, 4, 5):
        out[t] = b"".join(_enc(t, P) for P in secs[t])
    out[6] = _enc(6, secs[6])
    if prepared:
        lag = optau.prepare_phase2(secs, power)
        for t in (12, 13, 14, 15):
            out[t] = b"".join(_enc(t, P) for blk in lag[t] for P in blk)
    return binfile(out)


def oracle_prepare(buf) -> bytes:
    """env.prepare on the oracle: sections 12-15 recomputed from sections 2-5"""
    s = split(unprepared(buf))
    power = power_of(buf)
    pts = {t: [_dec(t, s[t][i:i + _size(t)]) for i in range(0, len(s[t]), _size(t))] for t in (2, 3, 4, 5)}
    lag = optau.prepare_phase2(pts, power)
    for t in (12, 13, 14, 15):
        s[t] = b"".join(_enc(t, P) for blk in lag[t] for P in blk)
    return binfile(s)


# ---- edits ----
def patch(buf, off, data):
    return bytes(buf[:off]) + bytes(data) + bytes(buf[off + len(data):])


def count(buf, t):
    return psecs(buf)[t][1] // _size(t)


def raw_point(buf, t, i):
    o = psecs(buf)[t][0] + i * _size(t)
    return bytes(buf[o:o + _size(t)])


def put_raw(buf, t, i, raw):
    assert len(raw) == _size(t) and i < count(buf, t)
    return patch(buf, psecs(buf)[t][0] + i * _size(t), raw)


def replaced(buf, t, i, k=0x1234567):
    """point i of section t := k * generator (a valid group element that does not belong there)"""
    new = _enc(t, bn.mul(_gen(t), k + 31 * t + i))
    assert new != raw_point(buf, t, i)
    return put_raw(buf, t, i, new)


def infinity(buf, t, i):
    return put_raw(buf, t, i, bytes(_size(t)))


def section_scaled(buf, t, k):
    for i in range(count(buf, t)):
        raw = raw_point(buf, t, i)
        if any(raw):
            buf = put_raw(buf, t, i, _enc(t, bn.mul(_dec(t, raw), k)))
    return buf


def off_curve(buf, t, i):
    """y + 1 (Montgomery form): canonical, not on the curve"""
    raw = raw_point(buf, t, i)
    yo = _size(t) // 2
    y = (int.from_bytes(raw[yo:yo + 32], "little") + 1) % Q
    return put_raw(buf, t, i, raw[:yo] + y.to_bytes(32, "little") + raw[yo + 32:])


def plus_q(buf, t, i):
    """x + q: the same point, coordinate not canonical"""
    raw = raw_point(buf, t, i)
    assert any(raw)
    x = int.from_bytes(raw[:32], "little") + Q
    return put_raw(buf, t, i, x.to_bytes(32, "little") + raw[32:])


def block_range(k):
    """positions of level k in a Lagrange section"""
    return range((1 << k) - 1, (2 << k) - 1)


def top_level(buf, t):
    return power_of(buf) + (1 if t == 12 else 0)


def swapped(buf, t, k):
    """the first two points of block k exchanged"""
    p = block_range(k)[0]
    a, b = raw_point(buf, t, p), raw_point(buf, t, p + 1)
    assert a != b
    return put_raw(put_raw(buf, t, p, b), t, p + 1, a)


def block_from(buf, other, t, k):
    for p in block_range(k):
        buf = put_raw(buf, t, p, raw_point(other, t, p))
    return buf


def bit_reversed(buf, t, k):
    pts = [raw_point(buf, t, p) for p in block_range(k)]
    rev = [pts[int(format(j, f"0{k}b")[::-1], 2)] for j in range(1 << k)]
    assert rev != pts
    for j, p in enumerate(block_range(k)):
        buf = put_raw(buf, t, p, rev[j])
    return buf


def tau_zero(buf, env):
    """tau = 0: every power but the zeroth is infinity, and the Lagrange sections say the same"""
    for t in (2, 3, 4, 5):
        for i in range(1, count(buf, t)):
            buf = infinity(buf, t, i)
    return env.prepare(unprepared(buf))


def alpha_zero(buf, env):
    for i in range(count(buf, 4)):
        buf = infinity(buf, 4, i)
    return env.prepare(unprepared(buf))


def lagrange_positions(buf, t):
    """one position in the lowest, a middle and the top level of Lagrange section t"""
    top = top_level(buf, t)
    mid = block_range(top // 2 + (1 if top < 4 else 0))
    return {"lowest": 0, "middle": mid[len(mid) // 2], "top": count(buf, t) - 1}


def table(power: int) -> dict:
    """name -> (edit(buf, env), checks that must fail, checks that must read "not run", the point
    the POINTS check must name or None); every other check passes."""
    assert power >= 2
    n = 1 << power
    T = {}

    def add(name, edit, fails, skipped=(), point=None):
        assert name not in T
        T[name] = (edit, set(fails), set(skipped), point)
    add("T0_not_generator", lambda b, e: replaced(b, 2, 0), {"STRUCTURE", "TAU_G1", "L_TAU_G1"})
    add("U0_not_generator", lambda b, e: replaced(b, 3, 0), {"STRUCTURE", "TAU_G2", "L_TAU_G2"})
    add("T1_infinity", lambda b, e: infinity(b, 2, 1), {"STRUCTURE", "TAU_G1", "TAU_G2", "L_TAU_G1"})
    add("tau_zero", tau_zero, {"STRUCTURE"})
    add("alpha_zero", alpha_zero, {"STRUCTURE"})
    # one power replaced: the chain and the Lagrange section both see it ...
    for t, last in ((2, 2 * n - 2), (3, n - 1), (4, n - 1), (5, n - 1)):
        for i in sorted({1, last // 2 + 1, last}):
            fails = {CHAIN[t], LAGRANGE[t + 10]}
            if (t, i) == (2, 1):
                fails.add("TAU_G2")                      # T[1] is TAU_G2's left-hand point
            if (t, i) == (3, 1):
                fails |= {"TAU_G1", "ALPHA_G1", "BETA_G1"}   # U[1] is every G1 chain's right-hand point
            add(f"sec{t}_point{i}_replaced", lambda b, e, t=t, i=i: replaced(b, t, i), fails)
        # ... and after `prepare phase2` of the tampered powers the chain alone does
        mid = last // 2 + 1
        add(f"sec{t}_point{mid}_replaced_reprepared",
            lambda b, e, t=t, i=mid: e.prepare(unprepared(replaced(b, t, i))), {CHAIN[t]})
    add("B0_replaced", lambda b, e: replaced(b, 5, 0), {"BETA_G1", "BETA_G2", "L_BETA_G1"})
    add("betaG2_replaced", lambda b, e: replaced(b, 6, 0), {"BETA_G2"})
    for t in (12, 13, 14, 15):
        for where in ("lowest", "middle", "top"):
            add(f"sec{t}_{where}_level_replaced",
                lambda b, e, t=t, w=where: replaced(b, t, lagrange_positions(b, t)[w]), {LAGRANGE[t]})
    add("sec12_block_swapped", lambda b, e: swapped(b, 12, power), {"L_TAU_G1"})
    add("sec14_block_swapped", lambda b, e: swapped(b, 14, power), {"L_ALPHA_G1"})
    add("sec12_block_of_another_tau", lambda b, e: block_from(b, e.other, 12, power + 1), {"L_TAU_G1"})
    add("sec13_block_of_another_tau", lambda b, e: block_from(b, e.other, 13, power), {"L_TAU_G2"})
    add("sec12_block_bit_reversed", lambda b, e: bit_reversed(b, 12, power + 1), {"L_TAU_G1"})
    add("sec15_block_bit_reversed", lambda b, e: bit_reversed(b, 15, power), {"L_BETA_G1"})
    # encodings: the section is named by the points check and takes no part in the later checks
    for t in (2, 3, 4, 5, 6, 12, 13, 14, 15):
        i = 0 if t == 6 else 2 if t < 12 else 4
        add(f"sec{t}_off_curve", lambda b, e, t=t, i=i: off_curve(b, t, i), {"POINTS"}, GATED[t], (t, i, 1))
    add("sec2_plus_q", lambda b, e: plus_q(b, 2, 3), {"POINTS"}, GATED[2], (2, 3, 1))
    add("sec13_plus_q", lambda b, e: plus_q(b, 13, 1), {"POINTS"}, GATED[13], (13, 1, 1))
    add("sec3_outside_g2", lambda b, e: put_raw(b, 3, 2, bn.g2_to_bytes_mont(twist_point_outside_g2())), {"POINTS"},
        GATED[3], (3, 2, 1))
    add("sec4_two_bad_points", lambda b, e: off_curve(off_curve(b, 4, n - 1), 4, 2), {"POINTS"}, GATED[4], (4, 2, 2))
    add("sec5_and_sec12_bad", lambda b, e: off_curve(off_curve(b, 12, 1), 5, 3), {"POINTS"}, GATED[5] | GATED[12],
        (5, 3, 1))
    return T


def expected(tab, name):
    """-> {check: state} of tamper `name`"""
    _, fails, skipped, _ = tab[name]
    return {c: "fail" if c in fails else "not run" if c in skipped else "pass" for c in CHECKS}


# files that must pass: name -> edit(buf, env); an unprepared file's Lagrange checks read "not run"
def alpha_scaled(buf, env):
    """sections 4 and 14 scaled by one constant: a valid file for another alpha"""
    return section_scaled(section_scaled(buf, 4, 0xABCDEF), 14, 0xABCDEF)


PASSES = {"as_built": lambda b, e: b, "alpha_scaled": alpha_scaled, "unprepared": lambda b, e: unprepared(b)}
