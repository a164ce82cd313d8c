"""`zkey check <circuit.r1cs> <pot_final.ptau> <circuit.zkey>`: is this .zkey the Groth16 proving
key of this .r1cs over this prepared .ptau, for some delta (and gamma)?

The reference proves with whatever `<c>_final.zkey` lies in the circuit directory and skips its
setup strings when one is there (tests/full_system_simulation.mjs:713-738); a client proves private
data with a key somebody else made, and Groth16 hides the witness only under a well-formed key.
The check (libzkfl zkfl_zkey_check, csrc/keycheck.hip; equations in include/zkfl.h and DESIGN.md §16)
tests the header against the ptau, every point's encoding, section 4 against the .r1cs as linear
maps, and sections 3, 5, 6, 7, 8, 9 by random linear combinations against the ptau's Lagrange
blocks.  It establishes that the key is the circuit's key over that ptau for SOME delta and gamma;
it does not establish who knows delta or snarkjs's csHash.  The ptau's own soundness -- are its
Lagrange blocks the Lagrange form of the powers of one tau? -- is `powersoftau check`'s question
(zkfl/ptaucheck.py); ``check_ptau=True`` / ``--check-ptau`` asks it first.
"""

from __future__ import annotations

import os
import sys

from . import native, r1cs_file
from .zkey import ptau_blocks


def _read(x) -> bytes:
    if isinstance(x, (bytes, bytearray, memoryview)):
        return bytes(x)
    with open(os.fspath(x), "rb") as f:
        return f.read()


def zkey_check(r1cs, ptau, zkey, ctx: native.Context | None = None, rho: bytes | None = None,
               sigma: bytes | None = None, check_ptau: bool = False):
    """r1cs, ptau, zkey: bytes or paths -> the check's report (``.ok``, ``.checks``, ``.error``).
    An unprepared or too small ptau raises ValueError as `groth16 setup` does; a malformed file or
    counts that disagree raise ZkflError.  rho / sigma are for tests (see native.R1cs.check_key).
    check_ptau: run the ptau check (zkfl/ptaucheck.py) first; a ptau that fails it ends the call
    with that check's report (a native.PtauReport, ``.ok`` False) and the key is not looked at."""
    r1cs_buf, zkey_buf = _read(r1cs), _read(zkey)
    ptau_buf = _read(ptau)
    blocks = ptau_blocks(r1cs_file.read_r1cs(r1cs_buf), ptau_buf)
    own = ctx is None
    if own:
        ctx = native.Context(int(os.environ.get("LOCAL_RANK", "0")))
    try:
        if check_ptau:
            prep = ctx.check_ptau(ptau_buf)
            if not prep.ok:
                return prep
        with native.R1cs(ctx, r1cs_buf) as cs:
            return cs.check_key(zkey_buf, blocks, rho, sigma)
    finally:
        if own:
            ctx.close()


def cli(args) -> int:
    """`zkey check` after its two words: exit 0 (the key passes), 1 (a check fails; one line per
    check on stdout, the first failing check on stderr) or 2 (unusable arguments, decided before
    the GPU is touched where the files alone show it)."""
    usage = "usage: zkey check <circuit.r1cs> <pot_final.ptau> <circuit.zkey> [--check-ptau]"
    check_ptau = "--check-ptau" in args
    args = [a for a in args if a != "--check-ptau"]
    if len(args) != 3:
        print(usage, file=sys.stderr)
        return 2
    for p in args:
        if not os.path.isfile(p):
            print(f"[ERROR] zkfl: zkey check: no such file: {p}\n{usage}", file=sys.stderr)
            return 2
    try:
        r1cs_buf = _read(args[0])
        ptau_buf = _read(args[1])
        blocks = ptau_blocks(r1cs_file.read_r1cs(r1cs_buf), ptau_buf)
    except (ValueError, OSError, AssertionError) as e:
        print(f"[ERROR] zkfl: zkey check: {e}", file=sys.stderr)
        return 2
    zkey_buf = _read(args[2])
    try:
        with native.Context(int(os.environ.get("LOCAL_RANK", "0"))) as ctx:
            if check_ptau:
                prep = ctx.check_ptau(ptau_buf)
                for line in prep.lines():
                    print(line)
                if not prep.ok:
                    print(f"[ERROR] zkfl: {prep.error}", file=sys.stderr)
                    return 1
            with native.R1cs(ctx, r1cs_buf) as cs:
                rep = cs.check_key(zkey_buf, blocks)
    except native.ZkflError as e:
        print(f"[ERROR] zkfl: zkey check: {e}", file=sys.stderr)
        return 2 if e.code in (-1, -2, -3, -4) else 1
    for line in rep.lines():
        print(line)
    if rep.ok:
        print("[INFO]  zkfl: ZKEY IS THE CIRCUIT'S KEY OVER THIS PTAU")
        return 0
    print(f"[ERROR] zkfl: {rep.error}", file=sys.stderr)
    return 1
