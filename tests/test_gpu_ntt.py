"""Every schedule of the coset NTT (csrc/ntt.hip ntt_coset_shift) against the C oracle, bit for bit,
on whole vectors -- run on an MI355X (-m gpu).

ntt_coset_shift picks its kernels from logn: up to 2^10 the two LDS kernels alone; 2^11 .. 2^20 a
column pass of k = logn - 10 stages, the fused LDS pair and a column pass back; above 2^20 radix-2
global stages around the unfused LDS kernels.  The tests run every logn of the first two, the batched
call the prover makes (three vectors, with and without a padded stride), and the third schedule both
at 2^21, where it is the natural one, and forced at small sizes (zkfl_debug_ntt_coset, col_max = 0).
Inputs (tests/ntt_vectors.py): random elements with the field's edge values in front, and whole
vectors of zero, r - 1, a constant, and 0 / r - 1 alternating.  The reference of every comparison is
cbaseline.coset_ntt, itself pinned to the Python oracle in tests/test_c_oracle.py.
"""
import ctypes
import functools

import pytest

import ntt_vectors as nv

pytestmark = pytest.mark.gpu

CACHE_MAX_LOGN = 17     # references above this are computed where they are used and dropped


def _oracle(data):
    from oracle import cbaseline
    return cbaseline.coset_ntt(data, cbaseline.default_threads())


def _seed(logn, v):
    return 1000 * logn + v


@functools.lru_cache(maxsize=None)
def _cached(logn, v):
    data = nv.random_vec(logn, _seed(logn, v))
    return data, _oracle(data)


def _vec_and_want(logn, v=0):
    """Random vector number v of size 2^logn and its coset transform by the C oracle (computed once
    per session for the sizes several tests share)."""
    if logn <= CACHE_MAX_LOGN:
        return _cached(logn, v)
    data = nv.random_vec(logn, _seed(logn, v))
    return data, _oracle(data)


def _check(got, want, what):
    if got == want:
        return
    assert len(got) == len(want), what
    bad = [i // 32 for i in range(0, len(want), 32) if got[i:i + 32] != want[i:i + 32]]
    pytest.fail(f"{what}: {len(bad)} of {len(want) // 32} elements differ from the oracle, the first at index {bad[0]}")


def _marker(g, count):
    return bytes((7 * i + 31 * g + 1) & 0xFF for i in range(32 * count))


# ---------------------------------------------------------------------------
# the default schedule at every size it takes: the LDS kernels at every tile size (logn <= 10), the
# column pass at every k = logn - 10 = 1 .. 10 (k = 10: one column per workgroup)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("logn", range(1, 21))
def test_ntt_default_schedule_matches_c_oracle(gpu_ctx, logn):
    data, want = _vec_and_want(logn)
    _check(gpu_ctx.ntt_coset(data), want, f"2^{logn} random, zkfl_ntt_coset")
    _check(gpu_ctx.debug_ntt_coset(data, logn), want, f"2^{logn} random, zkfl_debug_ntt_coset")
    for name, edge in nv.edge_vecs(logn).items():
        _check(gpu_ctx.debug_ntt_coset(edge, logn), _oracle(edge), f"2^{logn} {name}")


# ---------------------------------------------------------------------------
# batched as the prover calls it: three vectors, stride n
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("logn", [3, 10, 11, 12, 15, 17])
def test_ntt_batch_of_three_matches_c_oracle(gpu_ctx, logn):
    n = 1 << logn
    vecs = [_vec_and_want(logn, v) for v in range(3)]
    assert len({d for d, _ in vecs}) == 3
    out = gpu_ctx.debug_ntt_coset(b"".join(d for d, _ in vecs), logn, nvec=3)
    for v, (_, want) in enumerate(vecs):
        _check(out[32 * n * v:32 * n * (v + 1)], want, f"2^{logn} batch of 3, vector {v}")


# ---------------------------------------------------------------------------
# padded stride: the vectors are right and the gaps between them come back unchanged
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("logn,col_max", [(9, -1), (12, -1), (12, 0)])
def test_ntt_padded_stride_leaves_gaps(gpu_ctx, logn, col_max):
    n, pad = 1 << logn, 48
    vstride = n + pad
    vecs = [_vec_and_want(logn, v) for v in range(3)]
    gaps = [_marker(g, pad) for g in range(2)]
    data = vecs[0][0] + gaps[0] + vecs[1][0] + gaps[1] + vecs[2][0]
    out = gpu_ctx.debug_ntt_coset(data, logn, nvec=3, vstride=vstride, col_max=col_max)
    assert len(out) == len(data)
    for v, (_, want) in enumerate(vecs):
        _check(out[32 * vstride * v:32 * (vstride * v + n)], want, f"2^{logn} stride n + {pad}, vector {v}")
    for g in range(2):
        lo = 32 * (vstride * g + n)
        assert out[lo:lo + 32 * pad] == gaps[g], f"2^{logn} stride n + {pad}: gap {g} was written"


# ---------------------------------------------------------------------------
# the schedule of the domains above 2^20 (radix-2 global stages, unfused LDS kernels with more than
# one tile per vector), forced at small sizes: 2^11 has one global stage, 2^12 two (two twiddle strides)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nvec", [1, 3])
@pytest.mark.parametrize("logn", [11, 12, 14, 16])
def test_ntt_large_domain_schedule_at_small_sizes(gpu_ctx, logn, nvec):
    n = 1 << logn
    vecs = [_vec_and_want(logn, v) for v in range(nvec)]
    out = gpu_ctx.debug_ntt_coset(b"".join(d for d, _ in vecs), logn, nvec=nvec, col_max=0)
    for v, (_, want) in enumerate(vecs):
        _check(out[32 * n * v:32 * n * (v + 1)], want, f"2^{logn} col_max = 0, {nvec} vector(s), vector {v}")
    if nvec == 1:
        for name, edge in nv.edge_vecs(logn).items():
            _check(gpu_ctx.debug_ntt_coset(edge, logn, col_max=0), _oracle(edge), f"2^{logn} col_max = 0, {name}")


# ---------------------------------------------------------------------------
# ... and where it is the natural one (64 MB)
# ---------------------------------------------------------------------------
def test_ntt_large_domain_schedule_2_21(gpu_ctx):
    data, want = _vec_and_want(21)
    _check(gpu_ctx.ntt_coset(data), want, "2^21 random")


# ---------------------------------------------------------------------------
# argument errors: ZKFL_E_ARG, the buffer untouched
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("logn,nvec,vstride,col_max,null", [
    (0, 1, 1, -1, False), (28, 1, 1 << 28, -1, False), (3, 0, 8, -1, False), (3, 4, 8, -1, False),
    (3, 2, 7, -1, False), (3, 1, 7, -1, False), (3, 1, 8, -1, True), (3, 1, 8, 11, False)])
def test_ntt_argument_errors(gpu_ctx, logn, nvec, vstride, col_max, null):
    from zkfl import native
    before = _marker(5, 4 * 8)      # room for four vectors of 2^3
    buf = (ctypes.c_uint8 * len(before)).from_buffer_copy(before)
    rc = native.lib().zkfl_debug_ntt_coset(gpu_ctx.h, None if null else buf, logn, nvec, vstride, col_max)
    assert rc == -1                 # ZKFL_E_ARG
    assert bytes(buf) == before
    if nvec == 1 and col_max < 0 and not null and logn in (0, 28):
        assert native.lib().zkfl_ntt_coset(gpu_ctx.h, buf, logn) == -1
        assert bytes(buf) == before
