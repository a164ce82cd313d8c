"""`powersoftau check <pot.ptau>`: is this file a well-formed Powers of Tau for some tau, alpha and
beta, with sections 12-15 the Lagrange form of sections 2-5?

`groth16 setup` and `zkey check` read sections 12-15 of whatever `pot17_final.ptau` /
`pot14_final.ptau` they are handed (tests/full_system_simulation.mjs:677-695), and `zkey check` reads
the same blocks on both sides of its equations: a key made from a ptau whose Lagrange blocks are not
the Lagrange form of its powers, or whose powers are not the powers of one tau, passes it and is
unsound.  The check (libzkfl zkfl_ptau_check, csrc/ptaucheck.hip; equations in include/zkfl.h and
DESIGN.md §17) tests the generators, every point's encoding, the four power chains and betaG2 by
pairings of random combinations, and the four Lagrange sections against their power sections by one
random evaluation point each, streaming the file through the GPU in chunks.

It reads no contribution transcript: it establishes that the file is a Powers of Tau for SOME tau,
alpha and beta, not who knows them -- that is `powersoftau verify`'s question, which stays unserved
(the contribution records this framework writes are dev records, see zkfl/ptau.py).
"""

from __future__ import annotations

import mmap
import os
import sys

from . import native


class _Mapped:
    """A file mapped read-only (copy-on-write pages, never written): the check streams it from the
    page cache, so a multi-gigabyte ptau is not read into the process first."""

    def __init__(self, path):
        self.f = open(os.fspath(path), "rb")
        try:
            self.size = os.fstat(self.f.fileno()).st_size
            self.map = mmap.mmap(self.f.fileno(), 0, access=mmap.ACCESS_COPY) if self.size else b""
        except BaseException:
            self.f.close()
            raise

    def __enter__(self):
        return self.map

    def __exit__(self, *a):
        if self.size:
            try:
                self.map.close()
            except BufferError:   # a view is still alive: the map goes with it
                pass
        self.f.close()


def ptau_check(ptau, ctx: native.Context | None = None, rnd: bytes | None = None,
               chunk_points: int = 0) -> native.PtauReport:
    """ptau: bytes (or any buffer) or a path, which is mapped, not read -> the check's report
    (``.ok``, ``.checks``, ``.prepared``, ``.error``).  A malformed file raises ZkflError.  rnd and
    chunk_points are for tests (see native.Context.check_ptau)."""
    own = ctx is None
    if own:
        ctx = native.Context(int(os.environ.get("LOCAL_RANK", "0")))
    try:
        if isinstance(ptau, (bytes, bytearray, memoryview, mmap.mmap)):
            return ctx.check_ptau(ptau, rnd, chunk_points)
        with _Mapped(ptau) as buf:
            return ctx.check_ptau(buf, rnd, chunk_points)
    finally:
        if own:
            ctx.close()


USAGE = "usage: powersoftau check <pot.ptau>"


def cli(args) -> int:
    """`powersoftau check` after its two words: exit 0 (every check that ran holds; an unprepared
    file's Lagrange lines read "not run (not prepared)"), 1 (a check fails; one line per check on
    stdout, the first failing check on stderr) or 2 (unusable arguments or a malformed file,
    decided before the GPU is touched)."""
    if len(args) != 1:
        print(USAGE, file=sys.stderr)
        return 2
    path = args[0]
    if not os.path.isfile(path):
        print(f"[ERROR] zkfl: powersoftau check: no such file: {path}\n{USAGE}", file=sys.stderr)
        return 2
    try:
        with _Mapped(path) as buf:
            native.ptau_header(buf)   # the layout, host only
            with native.Context(int(os.environ.get("LOCAL_RANK", "0"))) as ctx:
                rep = ctx.check_ptau(buf)
    except native.ZkflError as e:
        print(f"[ERROR] zkfl: powersoftau check: {e}", file=sys.stderr)
        return 2 if e.code in (-1, -2, -3, -4) else 1
    except (OSError, ValueError) as e:
        print(f"[ERROR] zkfl: powersoftau check: {e}", file=sys.stderr)
        return 2
    for line in rep.lines():
        print(line)
    if rep.ok:
        what = "WITH ITS LAGRANGE SECTIONS" if rep.prepared else "(NOT PREPARED: NO LAGRANGE SECTIONS TO CHECK)"
        print(f"[INFO]  zkfl: PTAU IS A WELL-FORMED POWERS OF TAU {what}")
        return 0
    print(f"[ERROR] zkfl: {rep.error}", file=sys.stderr)
    return 1
