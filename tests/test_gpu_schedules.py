"""Every scheduler option of a context (csrc/objects.h SchedOpts) proves the same
bytes -- MI355X (-m gpu).

The options are read from the environment when a context is created, so each setting below opens
a context of its own, loads the key into it and proves fixed (witness, r, s) triples; the bar is
byte equality with the C oracle (oracle/c/groth16_ref.c), computed once for the module.

Circuit: sgd_verified(8, 4, 3, 1000), the smallest key that takes every schedule -- its B queries
share a sort and its domain is below 2^16, so by default it is a small key (run_front, joint
tails, the shorter-chain reduction) and with ZKFL_SMALL_LOGN=0 it runs the large-key chain
(run_chain: the stagger on the odd slot, B2's own tail, the throughput reduction).  A batch of
one takes the latency schedule (run_lowlat) unless ZKFL_LOWLAT=0.  The batch of six on three slots
gives every slot a proof launched kernel by kernel and then a graph replay with another witness
staged, unless ZKFL_GRAPH=0.
"""
import pytest

pytestmark = pytest.mark.gpu

PARAMS = (8, 4, 3, 1000)
SETTINGS = [
    {},
    {"ZKFL_GRAPH": "0"},
    {"ZKFL_STAGGER": "0"},
    {"ZKFL_LOWLAT": "0"},
    {"ZKFL_FAST_WSUM": "0"},
    {"ZKFL_SMALL_LOGN": "0"},
    {"ZKFL_SMALL_LOGN": "0", "ZKFL_GRAPH": "0"},
    {"ZKFL_SMALL_LOGN": "0", "ZKFL_STAGGER": "0"},
]
KNOBS = ("ZKFL_GRAPH", "ZKFL_STAGGER", "ZKFL_LOWLAT", "ZKFL_FAST_WSUM", "ZKFL_SMALL_LOGN")
N_BATCH = 6


def _le(x):
    return int(x).to_bytes(32, "little")


@pytest.fixture(scope="module")
def oracle_case(gpu_ctx):
    """The key, two witnesses (clients 1 and 2) and the oracle's answers: proof 0 is the single
    proof's (witness 0), proofs 1..6 the batch's (witnesses alternating, a distinct (r, s) each),
    h and the five MSMs those of witness 1."""
    from oracle import bn254 as bn
    from oracle import cbaseline
    from oracle import witness as ow
    from zkfl import circuits, clients, native, zkey
    b = circuits.build("sgd_verified", *PARAMS)
    zk = zkey.groth16_setup(b, gpu_ctx, zkey.Toxic(tau=0x5C4ED, alpha=0xA1, beta=0xB2, gamma=0xC3, delta=0xD4))
    wts = []
    for cid, seed in ((1, 12345), (2, 12347)):   # client 1 as test_proof_sgd_verified_reference_instance
        c = clients.Client(cid, 8, 4, 3, clients.JsLcg(seed))
        wts.append(zkey.wtns_bytes(ow.evaluate(b, c.training_input(8, 1000, 100000000)[0])))
    assert wts[0] != wts[1]
    rs = [_le(0x1234567) + _le(0x7654321), _le(bn.R - 1) + _le(bn.R - 2)]
    rs += [_le(0x1000 + 7 * i) + _le(0x2000 + 11 * i) for i in range(N_BATCH - 1)]
    which = [0] + [i % 2 for i in range(N_BATCH)]
    proofs = [cbaseline.prove(zk, wts[w], r) for w, r in zip(which, rs)]
    assert len(set(proofs)) == len(proofs)
    key = native.ProvingKey(gpu_ctx, zk)
    domain = key.domain_size
    key.close()
    _, ref_h, ref_parts = cbaseline.prove_parts(zk, wts[1], rs[0], domain)
    return zk, wts, rs, which, proofs, domain, ref_h, ref_parts


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: ",".join(f"{k}={v}" for k, v in s.items()) or "default")
def test_schedule_proves_the_oracle_bytes(oracle_case, monkeypatch, setting):
    from zkfl import native
    zk, wts, rs, which, proofs, domain, ref_h, ref_parts = oracle_case
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, value in setting.items():
        monkeypatch.setenv(name, value)
    with native.Context(0) as ctx:
        key = native.ProvingKey(ctx, zk)
        assert key.domain_size == domain and domain <= 1 << 16
        # (a) one proof alone
        proof, _ = key.prove(wts[which[0]], rs[0])
        assert proof == proofs[0], "a batch of one differs from the oracle"
        # (b) six proofs on the default three slots: slot i % 3 proves i and i + 3, with the other witness
        res = [key.upload(w) for w in wts]
        got = key.prove_batch([res[w] for w in which[1:]], b"".join(rs[1:]))
        for i in range(N_BATCH):
            assert got[i] == proofs[1 + i], f"batch proof {i} (slot {i % 3}) differs from the oracle"
        # (c) the large-key chain's parity hook: h and the five plain MSMs
        if setting.get("ZKFL_SMALL_LOGN") == "0":
            hs, parts = key.debug_parts(wts[1])
            assert hs == ref_h, "h (coset evaluations a*b - c) differ"
            for name in ("A", "B1", "B2", "C", "H"):
                assert parts[name] == ref_parts[name], f"MSM {name} differs"
