"""The Rescue-Prime kernels (sc_rescue_prime_hash_dev / sc_rescue_prime_trace_dev, csrc/rescue_prime.cuh) against the host mirror,
their argument checks, and the signature scheme built on them (fast_rpsss.FastRPSSS) against the reference's golden signature."""
import ctypes
import hashlib
import os
import pickle
import random

import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible"
    starkcore.init()


import starkcore as sc                              # noqa: E402
from algebra import Field, FieldElement             # noqa: E402
import fast_rpsss                                   # noqa: E402
import rescue_prime                                 # noqa: E402

P = Field.P_MAIN
SC_ERR_BAD_ARG = -6


@pytest.fixture(scope="module")
def rp():
    return rescue_prime.RescuePrime()


@pytest.fixture(scope="module")
def rpsss():
    return fast_rpsss.FastRPSSS()


@pytest.fixture
def seeded_urandom():
    genuine = os.urandom

    def install(seed):
        rng = random.Random(seed)
        os.urandom = lambda k: bytes(rng.getrandbits(8) for _ in range(k))
    yield install
    os.urandom = genuine


def inputs(seed, n):
    rng = random.Random(seed)
    xs = [rng.randrange(P) for _ in range(n)]
    for k, v in zip(range(min(n, 3)), (0, P - 1, 1)):
        xs[k] = v
    return xs


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_hash_and_trace_kernels_equal_the_host_mirror(rp, n):
    xs = inputs(n, n)
    vec = sc.DeviceVector.from_ints(xs)
    hashes = sc.unpack(rp.hash_device(vec).to_bytes())
    assert hashes == [rp.hash(FieldElement(x, rp.field)).value for x in xs]
    assert [h.value for h in rp.hash_batch([FieldElement(x, rp.field) for x in xs])] == hashes
    rows = rp.N + 1
    trace = sc.unpack(rp.trace_batch_device(vec).to_bytes())
    assert len(trace) == 2 * n * rows
    for k, x in enumerate(xs):
        want = rp.trace(FieldElement(x, rp.field))
        for s in range(rp.m):
            assert trace[(2 * k + s) * rows:(2 * k + s + 1) * rows] == [row[s].value for row in want], (k, s)


def test_kernels_at_a_million_inputs(rp):
    n, rows = 1 << 20, rp.N + 1
    rng = random.Random(20)
    vec = sc.DeviceVector.from_bytes(rng.randbytes(16 * n))          # 128-bit words: most are above p and are reduced on load
    picks = sorted(set([0, n - 1] + rng.sample(range(n), 256)))
    xs = vec.gather(picks)
    hashes = rp.hash_device(vec).gather(picks)
    assert hashes == [rp.hash(FieldElement(x % P, rp.field)).value for x in xs]
    trace = rp.trace_batch_device(vec)
    assert trace.n == 2 * n * rows
    for k, x in zip(picks[::16] + [n - 1], xs[::16] + [xs[-1]]):
        want = rp.trace(FieldElement(x % P, rp.field))
        got = trace.gather([(2 * k + s) * rows + t for s in range(rp.m) for t in range(rows)])
        assert got == [row[s].value for s in range(rp.m) for row in want], k


def test_empty_batch_and_bad_arguments(rp):
    lib = sc.lib()
    sentinel = sc.DeviceVector.from_ints([7, 8])
    before = sentinel.to_bytes()
    assert lib.sc_rescue_prime_hash_dev(None, 0, rp._params, rp.N, None, None) == 0
    assert lib.sc_rescue_prime_trace_dev(None, 0, rp._params, rp.N, None, None) == 0
    assert lib.sc_rescue_prime_hash_dev(sentinel.ptr, 0, rp._params, rp.N, sentinel.ptr, None) == 0
    sc.synchronize()
    assert sentinel.to_bytes() == before                                # n == 0 writes nothing
    assert rp.hash_batch([]) == [] and rp.hash_device(sc.DeviceVector(0)).n == 0
    src, dst = sc.DeviceVector.from_ints([1, 2]), sc.DeviceVector(2 * 2 * 28)
    too_big = sc.fe_bytes(P) + rp._params[16:]
    for entry in (lib.sc_rescue_prime_hash_dev, lib.sc_rescue_prime_trace_dev):
        assert entry(src.ptr, 2, rp._params, 0, dst.ptr, None) == SC_ERR_BAD_ARG
        assert entry(src.ptr, 2, rp._params + bytes(16 * 4), 28, dst.ptr, None) == SC_ERR_BAD_ARG
        assert entry(src.ptr, 2, None, rp.N, dst.ptr, None) == SC_ERR_BAD_ARG
        assert entry(None, 2, rp._params, rp.N, dst.ptr, None) == SC_ERR_BAD_ARG
        assert entry(src.ptr, 2, rp._params, rp.N, None, None) == SC_ERR_BAD_ARG
        assert entry(src.ptr, 2, too_big, rp.N, dst.ptr, None) == SC_ERR_BAD_ARG
        assert entry(None, 0, rp._params, 0, None, None) == SC_ERR_BAD_ARG
    sc.synchronize()


def test_trace_device_is_a_prover_trace(rp):
    x = FieldElement(987654321, rp.field)
    trace = rp.trace_device(x)
    assert len(trace) == rp.N + 1 and len(trace.columns) == rp.m
    want = rp.trace(x)
    assert [[trace.entry(t, s) for s in range(rp.m)] for t in range(rp.N + 1)] == want
    assert trace.entry(rp.N, 0) == rp.hash(x)


def test_keygen_batch_device_with_system_randomness(rpsss):
    sks, pks = rpsss.keygen_batch_device(1000)
    assert sks.n == pks.n == 1000
    picks = list(range(0, 1000, 97)) + [999]
    rp = rpsss.rp
    assert pks.gather(picks) == [rp.hash(FieldElement(v, rp.field)).value for v in sks.gather(picks)]
    assert all(v < P for v in sks.gather(picks))
    assert len(set(sks.gather(picks))) == len(picks)
    assert rpsss.keygen_batch(0) == ([], [])


# ---- the signature scheme against the reference's golden run (tests/golden/make_rpsss_golden.py)

@pytest.fixture(scope="module")
def golden_run(rpsss):
    g = load_golden("rpsss.json")
    genuine = os.urandom
    try:
        rng = random.Random(g["seed"])
        os.urandom = lambda k: bytes(rng.getrandbits(8) for _ in range(k))
        pairs = [rpsss.keygen() for _ in range(len(g["keys"]))]
        signature = rpsss.sign(pairs[g["signed_key"]][0], g["document"].encode())
    finally:
        os.urandom = genuine
    return g, pairs, signature


def test_keygen_matches_the_reference(rpsss, golden_run, seeded_urandom):
    g, pairs, _ = golden_run
    assert [[str(sk.value), str(pk.value)] for sk, pk in pairs] == g["keys"]
    seeded_urandom(g["seed"])
    sks, pks = rpsss.keygen_batch(len(g["keys"]))
    assert [[str(sk.value), str(pk.value)] for sk, pk in zip(sks, pks)] == g["keys"]


def test_signature_is_the_reference_signature(golden_run):
    g, _, signature = golden_run
    assert len(signature) == g["signature_len"]
    assert hashlib.sha256(signature).hexdigest() == g["signature_sha256"]


def test_host_trace_signature_is_the_same(rpsss, golden_run, seeded_urandom):
    g, pairs, signature = golden_run
    seeded_urandom(g["seed"])
    for _ in range(len(g["keys"])):
        os.urandom(17)
    try:
        fast_rpsss.FastRPSSS.SIGN_ON_DEVICE = False
        again = rpsss.sign(pairs[g["signed_key"]][0], g["document"].encode())
    finally:
        fast_rpsss.FastRPSSS.SIGN_ON_DEVICE = True
    assert again == signature


def test_verify_and_verify_batch(rpsss, golden_run):
    g, pairs, signature = golden_run
    doc = g["document"].encode()
    pk = pairs[g["signed_key"]][1]
    other_pk = pairs[1][1]
    objects = pickle.loads(signature)
    bad = list(objects)
    bad[-2] = bad[-2] + Field.main().one()                 # one opened leaf changed
    tampered = pickle.dumps(bad)
    cases = [(pk, doc, signature), (pk, doc + b"!", signature), (other_pk, doc, signature), (pk, doc, tampered),
             (pk, doc, b"not a signature")]

    def host(args):
        try:
            return rpsss.verify(*args) == True          # noqa: E712
        except Exception:
            return False
    want = [host(c) for c in cases]
    assert want == [True, False, False, False, False]
    assert rpsss.verify_batch([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]) == want
    assert rpsss.verify_batch([pk] * 3, [doc] * 3, [signature] * 3) == [True] * 3
    assert rpsss.verify_batch([], [], []) == []
