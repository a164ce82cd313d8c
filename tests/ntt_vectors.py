"""Input vectors for the coset-NTT tests (tests/test_c_oracle.py, tests/test_gpu_ntt.py): standard-form
Fr elements as bytes, built without a Python loop over the elements."""
import random

from oracle import bn254 as bn

R = bn.R
# the two ends of the field, the largest power of two below r, and the middle
EDGES = (0, 1, R - 1, R - 2, 1 << 253, (R - 1) // 2)
_MASK5 = bytes(i & 0x1F for i in range(256))
ALTERNATING_MAX_LOGN = 12


def le(x):
    return int(x).to_bytes(32, "little")


def random_vec(logn, seed):
    """2^logn uniform elements below 2^253 (< r: the top byte masked to 5 bits), the first slots
    overwritten by EDGES (as many as fit)."""
    n = 1 << logn
    b = bytearray(random.Random(seed).randbytes(32 * n))
    b[31::32] = b[31::32].translate(_MASK5)
    k = min(n, len(EDGES))
    b[:32 * k] = b"".join(le(e) for e in EDGES[:k])
    return bytes(b)


def edge_vecs(logn):
    """Whole-vector edge inputs by byte repetition: name -> bytes."""
    n = 1 << logn
    out = {"zero": bytes(32 * n), "all_r_minus_1": le(R - 1) * n, "constant": le(EDGES[5] + 12345) * n}
    if logn <= ALTERNATING_MAX_LOGN:
        out["alternating"] = (le(0) + le(R - 1)) * (n // 2)
    return out


def ints(data):
    return [int.from_bytes(data[i:i + 32], "little") for i in range(0, len(data), 32)]
