"""snarkjs-compatible Groth16 surface backed by libzkfl (HIP).

Mirrors the snarkjs API/CLI the reference harness drives:
  ``groth16.prove(zkey, wtns)``            <- ``snarkjs groth16 prove`` (tests/full_system_simulation.mjs:773-776)
  ``groth16.fullProve(input, circuit, zkey)`` <- snarkjs ``groth16.fullProve`` (witness + prove)
  ``wtns_calculate(circuit, input)``       <- ``generate_witness.cjs`` / ``snarkjs wtns calculate`` (:758-767)
  ``export_verification_key(zkey)``        <- ``snarkjs zkey export verificationkey`` (:732-735)
  ``r1cs_info(circuit)``                   <- ``snarkjs r1cs info`` (tests/test_verified_gradient.mjs:351-356)
  ``verify(vkey, public, proof)``          <- ``snarkjs groth16 verify`` (:865-868), on the GPU
  ``wtns_check(r1cs, wtns)``               <- ``snarkjs wtns check <c.r1cs> <w.wtns>`` (snarkjs ``wtns.check``), on the GPU
  ``zkey_check(r1cs, ptau, zkey)``         the key against its circuit and ptau (no snarkjs counterpart), on the GPU
  ``ptau_check(ptau)``                     the ptau's powers and Lagrange sections (no transcript: not ``powersoftau verify``), on the GPU
Outputs are snarkjs's JSON shapes: proof.json = {pi_a, pi_b, pi_c, protocol, curve} with
decimal strings, public.json = list of decimal strings (witness[1..nPublic]).
"""

from __future__ import annotations

import hashlib
import os

from . import native, wprog
from .field import Q
from .zkey import read_wtns, zkey_header

_RINV_Q = pow(2 ** 256, Q - 2, Q)


def _read(x) -> bytes:
    if isinstance(x, (bytes, bytearray, memoryview)):
        return bytes(x)
    with open(os.fspath(x), "rb") as f:
        return f.read()


def _le(b: bytes, i: int) -> int:
    return int.from_bytes(b[32 * i:32 * i + 32], "little")


def proof_to_json(proof: bytes) -> dict:
    """256-byte C-ABI proof -> snarkjs proof.json object."""
    v = [str(_le(proof, i)) for i in range(8)]
    return {
        "pi_a": [v[0], v[1], "1"],
        "pi_b": [[v[2], v[3]], [v[4], v[5]], ["1", "0"]],
        "pi_c": [v[6], v[7], "1"],
        "protocol": "groth16",
        "curve": "bn128",
    }


def proof_from_json(p: dict) -> bytes:
    vals = [p["pi_a"][0], p["pi_a"][1], p["pi_b"][0][0], p["pi_b"][0][1], p["pi_b"][1][0], p["pi_b"][1][1],
            p["pi_c"][0], p["pi_c"][1]]
    return b"".join(int(x).to_bytes(32, "little") for x in vals)


def _mont_to_std_q(b: bytes):
    return [int.from_bytes(b[i:i + 32], "little") * _RINV_Q % Q for i in range(0, len(b), 32)]


def export_verification_key(zkey, alphabeta: bool = True, ctx: native.Context | None = None) -> dict:
    """snarkjs ``zkey export verificationkey``.  ``vk_alphabeta_12`` = e(alpha1, beta2) is
    computed with the GPU pairing (``zkfl_pairing``); pass ``alphabeta=False`` to skip it (the
    verifier does not read it: snarkjs verify uses the 4-pair product)."""
    h = zkey_header(_read(zkey))

    def g1(b):
        x, y = _mont_to_std_q(b)
        return [str(x), str(y), "1"]

    def g2(b):
        x0, x1, y0, y1 = _mont_to_std_q(b)
        return [[str(x0), str(x1)], [str(y0), str(y1)], ["1", "0"]]

    vk = {
        "protocol": "groth16", "curve": "bn128", "nPublic": h["nPublic"],
        "vk_alpha_1": g1(h["alpha1"]), "vk_beta_2": g2(h["beta2"]), "vk_gamma_2": g2(h["gamma2"]),
        "vk_delta_2": g2(h["delta2"]),
    }
    if alphabeta:
        c = ctx or _prover().ctx
        gt = c.pairing(_g1_bytes(vk["vk_alpha_1"]), _g2_bytes(vk["vk_beta_2"]))
        v = [str(_le(gt, i)) for i in range(12)]
        vk["vk_alphabeta_12"] = [[v[6 * i + 2 * j:6 * i + 2 * j + 2] for j in range(3)] for i in range(2)]
    vk["IC"] = [g1(p) for p in h["IC"]]
    return vk


def _g1_bytes(p) -> bytes:
    """snarkjs JSON G1 [x, y, z] (z = "1", or "0" for infinity) -> 64 B std LE (infinity = zeros)."""
    if int(p[2]) == 0:
        return bytes(64)
    assert int(p[2]) == 1, "projective JSON points are not supported"
    return int(p[0]).to_bytes(32, "little") + int(p[1]).to_bytes(32, "little")


def _g2_bytes(p) -> bytes:
    if int(p[2][0]) == 0 and int(p[2][1]) == 0:
        return bytes(128)
    assert int(p[2][0]) == 1 and int(p[2][1]) == 0, "projective JSON points are not supported"
    return b"".join(int(x).to_bytes(32, "little") for x in (p[0][0], p[0][1], p[1][0], p[1][1]))


def vk_bytes(vk: dict) -> bytes:
    """vkey.json -> the C-ABI vk image (include/zkfl.h, zkfl_groth16_verify)."""
    return (int(vk["nPublic"]).to_bytes(4, "little") + _g1_bytes(vk["vk_alpha_1"]) + _g2_bytes(vk["vk_beta_2"])
            + _g2_bytes(vk["vk_gamma_2"]) + _g2_bytes(vk["vk_delta_2"]) + b"".join(_g1_bytes(p) for p in vk["IC"]))


def public_bytes(public) -> bytes:
    """public.json (decimal strings) -> npub x 32 B std LE.  Values >= 2^256 cannot be encoded
    and are rejected here; values in [r, 2^256) reach the verifier, which reports them invalid."""
    return b"".join(int(x).to_bytes(32, "little") for x in public)


def wtns_calculate(circuit, inputs: dict) -> bytes:
    """Witness generation on the GPU (circom WASM + generate_witness.cjs replacement) -> .wtns
    bytes; an unsatisfied assert raises ZkflError with code ZKFL_E_CONSTRAINT (-7)."""
    return _prover().wtns_calculate(circuit, inputs)


def r1cs_info(circuit) -> dict:
    return {
        "curve": "bn-128", "wires": circuit.n_wires, "constraints": circuit.n_constraints,
        "privateInputs": circuit.n_prv_in, "publicInputs": circuit.n_pub_in,
        "outputs": circuit.n_pub_out, "labels": circuit.n_wires,
    }


class Prover:
    """Keeps one device context and device-resident proving keys (load once, prove many:
    the reference's artifact caching, SURVEY.md §5 checkpoint/resume)."""

    def __init__(self, device: int = 0):
        self.ctx = native.Context(device)
        self._keys = {}
        self._vkeys = {}
        self._progs = {}

    def program(self, circuit) -> native.WitnessProgram:
        """The circuit's compiled witness program, loaded once (the .wasm's role)."""
        p = self._progs.get(id(circuit))
        if p is None:
            p = (circuit, native.WitnessProgram(self.ctx, wprog.compile_program(circuit)))
            self._progs[id(circuit)] = p
        return p[1]

    def wtns_calculate(self, circuit, inputs: dict) -> bytes:
        return self.program(circuit).compute([wprog.input_bytes(circuit, inputs)])[0]

    def key(self, zkey) -> native.ProvingKey:
        buf = _read(zkey)
        digest = hashlib.sha256(buf).digest()
        k = self._keys.get(digest)
        if k is None:
            k = native.ProvingKey(self.ctx, buf)
            self._keys[digest] = k
        return k

    def prove(self, zkey, wtns, rs: bytes | None = None, r1cs=None, check_key=None):
        """-> (proof.json dict, public.json list).  r1cs (bytes or path): the witness is checked
        against it first, and one that does not satisfy it raises ZkflError(ZKFL_E_CONSTRAINT)
        instead of yielding a proof that cannot verify.  check_key = (r1cs, ptau): the key is
        checked against them before it is loaded (zkfl/keycheck.py); one that fails raises
        ZkflError(ZKFL_E_KEY)."""
        wtns = _read(wtns)
        if check_key is not None:
            from . import keycheck
            rep = keycheck.zkey_check(check_key[0], check_key[1], zkey, self.ctx)
            if not rep.ok:
                raise native.ZkflError(-8, rep.error)
        if r1cs is not None:
            with native.R1cs(self.ctx, _read(r1cs)) as cs:
                if not cs.check([wtns], reports=False):
                    raise native.ZkflError(-7, cs.last_error)
        proof, pub = self.key(zkey).prove(wtns, rs)
        return proof_to_json(proof), [str(x) for x in pub]

    def full_prove(self, inputs: dict, circuit, zkey, rs: bytes | None = None):
        return self.prove(zkey, self.wtns_calculate(circuit, inputs), rs)

    def verify(self, vk: dict, public, proof: dict) -> bool:
        return self.ctx.verify(vk_bytes(vk), public_bytes(public), proof_from_json(proof))

    def verify_batch(self, vk: dict, publics, proofs) -> list:
        """Many proofs against one key in one launch (the server's per-round check)."""
        return self.ctx.verify_batch(vk_bytes(vk), b"".join(public_bytes(p) for p in publics),
                                     b"".join(proof_from_json(p) for p in proofs), int(vk["nPublic"]))

    def load_vkey(self, vk: dict) -> native.VerifyingKey:
        """vkey.json dict -> a device-resident verification key (loaded once per distinct key)."""
        image = vk_bytes(vk)
        digest = hashlib.sha256(image).digest()
        k = self._vkeys.get(digest)
        if k is None or not k.h:
            k = native.VerifyingKey(self.ctx, image)
            self._vkeys[digest] = k
        return k

    def verify_multi(self, jobs, schedule: str = "auto") -> list:
        """jobs: [(vkey.json dict or load_vkey handle, publicSignals, proof.json dict)] -> [bool]:
        a round's proofs, each against its own resident key, in one call (the server's loop,
        tests/full_system_simulation.mjs:1298-1343)."""
        return self.ctx.verify_multi(
            [(vk if isinstance(vk, native.VerifyingKey) else self.load_vkey(vk), public_bytes(pub),
              proof_from_json(proof)) for vk, pub, proof in jobs], schedule)

    def verify_round(self, jobs, z=None):
        """verify_multi's jobs -> ([bool], report dict), answered for the whole round by one random
        combination with one final exponentiation; when it fails, the exact verdicts come from the
        per-proof path (Context.verify_round).  z: for tests only."""
        return self.ctx.verify_round(
            [(vk if isinstance(vk, native.VerifyingKey) else self.load_vkey(vk), public_bytes(pub),
              proof_from_json(proof)) for vk, pub, proof in jobs], z)

    def verify_round_narrow(self, jobs, z=None, group: int = 0):
        """verify_round's jobs and verdicts -> ([bool], narrow report dict); a failed round is
        narrowed to the groups whose own combination fails, and only their jobs go to the
        per-proof path (Context.verify_round_narrow).  group 0: the production policy."""
        return self.ctx.verify_round_narrow(
            [(vk if isinstance(vk, native.VerifyingKey) else self.load_vkey(vk), public_bytes(pub),
              proof_from_json(proof)) for vk, pub, proof in jobs], z, group)

    def close(self):
        for k in list(self._keys.values()) + list(self._vkeys.values()):
            k.close()
        self._keys.clear()
        self._vkeys.clear()
        for _, p in self._progs.values():
            p.close()
        self._progs.clear()
        self.ctx.close()


_default = None


def _prover() -> Prover:
    global _default
    if _default is None:
        _default = Prover(int(os.environ.get("LOCAL_RANK", "0")))
    return _default


def prove(zkey, wtns, rs: bytes | None = None, r1cs=None, check_key=None):
    return _prover().prove(zkey, wtns, rs, r1cs=r1cs, check_key=check_key)


def wtns_check_report(r1cs, wtns, ctx: native.Context | None = None) -> native.Report:
    """The witness (.wtns bytes or path) against the circuit's .r1cs (bytes or path) -> the check's
    report: n_failed, the first failing constraint and its a, b, c values."""
    with native.R1cs(ctx or _prover().ctx, _read(r1cs)) as cs:
        return cs.check([_read(wtns)])[0]


def wtns_check(r1cs, wtns, ctx: native.Context | None = None) -> bool:
    """snarkjs ``wtns.check(r1csFileName, wtnsFileName)`` -> bool: every constraint of the .r1cs
    holds for the witness (checked on the GPU).  A malformed file, or a witness of another length
    than the circuit's wires, raises ZkflError."""
    return wtns_check_report(r1cs, wtns, ctx).ok


def zkey_check(r1cs, ptau, zkey, ctx: native.Context | None = None, check_ptau: bool = False):
    """Is ``zkey`` the Groth16 proving key of ``r1cs`` over the prepared ``ptau`` (bytes or paths),
    for some delta and gamma?  -> the report (``.ok``, ``.checks``, ``.error``), checked on the GPU
    (zkfl/keycheck.py).  No snarkjs counterpart: ``zkey verify`` asserts a contribution transcript.
    check_ptau: run ``ptau_check`` on the ptau first and stop with its report if it fails."""
    from . import keycheck
    return keycheck.zkey_check(r1cs, ptau, zkey, ctx or _prover().ctx, check_ptau=check_ptau)


def ptau_check(ptau, ctx: native.Context | None = None) -> native.PtauReport:
    """Is ``ptau`` (bytes, or a path, which is mapped) a well-formed Powers of Tau for some tau,
    alpha and beta, with sections 12-15 the Lagrange form of sections 2-5?  -> the report (``.ok``,
    ``.checks``, ``.prepared``, ``.error``), checked on the GPU (zkfl/ptaucheck.py).  It reads no
    contribution transcript: not ``powersoftau verify``."""
    from . import ptaucheck
    return ptaucheck.ptau_check(ptau, ctx or _prover().ctx)


def fullProve(inputs: dict, circuit, zkey, rs: bytes | None = None):  # noqa: N802 (snarkjs name)
    return _prover().full_prove(inputs, circuit, zkey, rs)


def verify(vk: dict, public, proof: dict) -> bool:
    """snarkjs ``groth16.verify(vKey, publicSignals, proof)`` -> bool (GPU pairing check)."""
    return _prover().verify(vk, public, proof)


def load_vkey(vk: dict) -> native.VerifyingKey:
    """A vkey.json dict made device-resident on the default prover (Prover.load_vkey)."""
    return _prover().load_vkey(vk)


def verify_multi(jobs, schedule: str = "auto") -> list:
    """[(vKey or load_vkey handle, publicSignals, proof)] -> [bool] in one call (Prover.verify_multi)."""
    return _prover().verify_multi(jobs, schedule)


def verify_round(jobs, z=None):
    """verify_multi's jobs -> ([bool], report dict) by one random combination (Prover.verify_round)."""
    return _prover().verify_round(jobs, z)


def verify_round_narrow(jobs, z=None, group: int = 0):
    """verify_round with a failed round narrowed to its bad groups (Prover.verify_round_narrow)."""
    return _prover().verify_round_narrow(jobs, z, group)


__all__ = ["prove", "fullProve", "verify", "verify_multi", "verify_round", "verify_round_narrow", "load_vkey", "Prover", "proof_to_json", "proof_from_json", "export_verification_key",
           "vk_bytes", "public_bytes", "wtns_calculate", "r1cs_info", "read_wtns", "wtns_check",
           "wtns_check_report", "zkey_check", "ptau_check"]
