"""What the NTT's product-free butterflies (csrc/ntt.hip) rest on, checked on the CPU against Python
big integers through tools/fr_check.cpp, which drives csrc/field.h's own fp_add / fp_sub / fp_mul
(on the host the column multiply-add is plain C++, everything else is the device's code).

The span-1 stages, and the j = 0 butterflies of the span-2 stages, multiply by tw[0], which
k_ntt_twiddles leaves as fp_one (the Montgomery one) exactly.  Dropping that product is bit-exact
iff fp_mul(x, one) == x for every x those stages see, which holds for x < r (the product is
x R R^-1 mod r, fully reduced) and fails for r <= x < 2^256 (the product comes back reduced, x does
not).  So the argument needs every value in a tile to be fully reduced:
  * fp_add and fp_sub of reduced operands are reduced (the butterflies' sums and differences);
  * fp_mul with one operand below r is reduced whatever the other is (the twiddle and scale
    products, and fp_to_mont of a caller's raw 256-bit words: what enters the transform).
"""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "verifiable-federated-training-with-zero-knowledge-proofs-zk-fl-_amd")
HIPCC = "/opt/rocm/bin/hipcc"
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MONT = (1 << 256) % R
MINV = pow(MONT, -1, R)
EDGES = [0, 1, 2, R - 1, R - 2, MONT, R - MONT, (1 << 253), (1 << 253) - 1, (R - 1) // 2, (R + 1) // 2,
         (1 << 32) - 1, 1 << 32, (1 << 224), R - (1 << 32)]


@pytest.fixture(scope="module")
def fr(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("fr") / "fr_check")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-I" + os.path.join(PKG, "csrc"), "-o", out,
                    os.path.join(ROOT, "tools", "fr_check.cpp")], check=True, capture_output=True)

    def run(lines):
        r = subprocess.run([out], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
        return [int(ln, 16) for ln in r.stdout.split()]
    return run


def hx(v):
    return f"{v:064x}"


def reduced_values(seed, count):
    rng = random.Random(seed)
    return EDGES + [rng.randrange(R) for _ in range(count)]


def test_montgomery_one(fr):
    assert fr(["one"]) == [MONT]


def test_mul_by_one_is_identity_on_reduced(fr):
    vals = reduced_values(1, 2000)
    assert fr([f"mulone {hx(v)}" for v in vals]) == vals
    assert fr([f"mul {hx(MONT)} {hx(v)}" for v in vals]) == vals


def test_mul_by_one_reduces_unreduced(fr):
    """The condition is needed: an unreduced x does not come back unchanged."""
    rng = random.Random(2)
    vals = [R, R + 1, (1 << 256) - 1, 2 * R - 1, 2 * R] + [rng.randrange(R, 1 << 256) for _ in range(200)]
    got = fr([f"mulone {hx(v)}" for v in vals])
    assert got == [v % R for v in vals]
    assert all(g != v for g, v in zip(got, vals))


def test_add_sub_of_reduced_are_reduced(fr):
    vals = reduced_values(3, 300)
    rng = random.Random(4)
    pairs = [(a, b) for a in EDGES for b in EDGES] + [(rng.choice(vals), rng.choice(vals)) for _ in range(2000)]
    assert fr([f"add {hx(a)} {hx(b)}" for a, b in pairs]) == [(a + b) % R for a, b in pairs]
    assert fr([f"sub {hx(a)} {hx(b)}" for a, b in pairs]) == [(a - b) % R for a, b in pairs]


def test_products_are_reduced(fr):
    """One operand below r: the product is a b R^-1 mod r, below r, also for a raw 256-bit other
    operand (fp_to_mont of a caller's words; the twiddles and the coset table are below r)."""
    rng = random.Random(5)
    vals = reduced_values(6, 300)
    raw = [(1 << 256) - 1, R, 2 * R, 5 * R + 3] + [rng.randrange(1 << 256) for _ in range(300)]
    pairs = [(a, b) for a in EDGES for b in EDGES] + [(rng.choice(vals), rng.choice(vals)) for _ in range(1500)]
    pairs += [(a, rng.choice(vals)) for a in raw]
    assert fr([f"mul {hx(a)} {hx(b)}" for a, b in pairs]) == [a * b * MINV % R for a, b in pairs]
    assert fr([f"tomont {hx(a)}" for a in raw + vals]) == [a * MONT % R for a in raw + vals]
    assert fr([f"frommont {hx(a)}" for a in vals]) == [a * MINV % R for a in vals]


def test_fused_boundary_equals_three_steps(fr):
    """The pair (2t, 2t + 1) through the inverse span-1 stage, the coset scale and the forward span-1
    stage: two products give what the four (two of them by one) gave."""
    rng = random.Random(7)
    vals = reduced_values(8, 100)
    cases = [tuple(rng.choice(vals) for _ in range(4)) for _ in range(500)]
    lines = []
    for u, w, s0, s1 in cases:
        x0, x1 = (u + w) % R, (u - w) % R
        lines += [f"mulone {hx(x1)}", f"mul {hx(x0)} {hx(s0)}", f"mul {hx(x1)} {hx(s1)}"]
    got = fr(lines)
    for k, (u, w, s0, s1) in enumerate(cases):
        x1_one, y0, y1 = got[3 * k:3 * k + 3]
        assert x1_one == (u - w) % R                      # the inverse stage's product by one
        assert y0 == (u + w) * s0 * MINV % R and y1 == (u - w) * s1 * MINV % R
    y1s = got[2::3]
    assert fr([f"mulone {hx(y)}" for y in y1s]) == y1s    # the forward stage's product by one
