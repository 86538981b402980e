"""Membership proofs for Rescue-Prime Merkle trees on the GPU: the path-trace kernels (sc_rescue_merkle_path_trace_dev;
csrc/rescue_merkle.cuh and rescue_merkle.hip) on the cases of tests/rescue_membership_cases.py in both forms, against the plain-integer
model, and rescue_membership.RescueMembership over them: prove, verify, the batched forms, proofs from a resident tree.

Traces land in windows of larger buffers filled with a sentinel; afterwards the window equals the model and the guards hold the
sentinel.  Everything is compared exactly."""
import ctypes
import functools
import hashlib
import os
import random

import pytest

from conftest import load_golden
import rescue_membership_cases as mc
import rescue_wide_cases as wc

pytestmark = pytest.mark.gpu

import starkcore as sc                              # noqa: E402
import rescue_prime                                 # noqa: E402
import rescue_merkle                                # noqa: E402
import rescue_membership                            # noqa: E402
from algebra import Field, FieldElement             # noqa: E402
from fast_stark import FastStark, DeviceTrace       # noqa: E402

P = mc.P
SC_OK, SC_ERR_BAD_ARG = 0, -6
GUARD = 64
SENTINEL_INT = random.Random(0x3E3B).randrange(P + 1, 1 << 128)      # no canonical residue: the kernel never writes it
SENTINEL = sc.fe_bytes(SENTINEL_INT)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert sc.device_count() > 0, "no GPU visible"
    sc.init()


@pytest.fixture(autouse=True)
def _restore_key():
    yield
    rescue_merkle.set_split_max_nodes(-1)


@pytest.fixture
def seeded(monkeypatch):
    def seed(value):
        rng = random.Random(value)
        monkeypatch.setattr(os, "urandom", lambda k: bytes(rng.getrandbits(8) for _ in range(k)))
    return seed


class Window:
    """`elems` elements GUARD elements inside a device vector of sentinels"""

    def __init__(self, elems):
        self.elems = elems
        self.before = SENTINEL * (elems + 2 * GUARD)
        self.vec = sc.DeviceVector.from_bytes(self.before)
        self.ptr = self.vec.ptr + 16 * GUARD

    def read(self):
        raw = self.vec.to_bytes()
        self.guards_hold = raw[:16 * GUARD] == SENTINEL * GUARD and raw[16 * (GUARD + self.elems):] == SENTINEL * GUARD
        self.untouched = raw == self.before
        return wc.unpack(raw[16 * GUARD:16 * (GUARD + self.elems)])


def params_of(m, rounds):
    return wc.params_bytes(*wc.seeded_params(m, rounds))


def trace_call(m, capacity, d, rounds, depth, k, leaves, indices, paths, out_ptr, stream=None):
    idx = (ctypes.c_uint64 * max(k, 1))(*indices)
    return sc.lib().sc_rescue_merkle_path_trace_dev(leaves, idx, paths, k, depth, d, m, m - capacity, params_of(m, rounds), rounds, out_ptr, stream)


# ---- the kernels ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", mc.SHAPES)
def test_every_trace_equals_the_model_in_both_forms(shape):
    for m, capacity, d, rounds, depth, k, kind in mc.kernel_cases():
        if (m, capacity, d) != shape:
            continue
        leaves, indices, paths = mc.packed_inputs(m, d, depth, kind, k)
        want = mc.expected_matrix(m, capacity, d, rounds, depth, kind, k)
        assert len(want) == k * mc.registers(m, d) * mc.rows_of(depth, rounds)
        for key in mc.KEYS:
            rescue_merkle.set_split_max_nodes(key)
            out = Window(len(want))
            assert trace_call(m, capacity, d, rounds, depth, k, leaves, indices, paths, out.ptr) == SC_OK, sc.lib().sc_last_error()
            sc.synchronize()
            got = out.read()
            assert out.guards_hold, (rounds, depth, k, kind, key)
            assert got == want, (rounds, depth, k, kind, key, "first element that differs", next(i for i in range(len(want)) if got[i] != want[i]))


def test_on_a_callers_stream_and_large_inputs():
    """a caller's stream; and inputs beyond what travels as kernel arguments (the staged copy): depth 63 paths of 17 items"""
    import torch
    stream = torch.cuda.Stream(device=torch.device("cuda", 0))
    handle = ctypes.c_void_p(stream.cuda_stream)
    m, capacity, d, rounds, depth, kind, k = 4, 1, 1, 1, 63, "random", 17
    leaves, indices, paths = mc.packed_inputs(m, d, depth, kind, k)
    assert len(paths) > 8192
    want = mc.expected_matrix(m, capacity, d, rounds, depth, kind, k)
    for key in mc.KEYS:
        rescue_merkle.set_split_max_nodes(key)
        out = Window(len(want))
        sc.synchronize()
        assert trace_call(m, capacity, d, rounds, depth, k, leaves, indices, paths, out.ptr, handle) == SC_OK, sc.lib().sc_last_error()
        torch.cuda.synchronize()
        assert out.read() == want and out.guards_hold


def good():
    m, rounds = 6, 2
    return dict(m=m, capacity=1, d=2, rounds=rounds, depth=3, k=2, indices=[1, 7], params=params_of(m, rounds), null=())


def p_at(c, word):
    return dict(params=c["params"][:16 * word] + sc.fe_bytes(P) + c["params"][16 * (word + 1):])


REFUSALS = [
    ("m = 1", lambda c: dict(m=1)),
    ("m = 9", lambda c: dict(m=9)),
    ("rate = 1", lambda c: dict(capacity=c["m"] - 1)),
    ("rate = m", lambda c: dict(capacity=0)),
    ("digest_len = 0", lambda c: dict(d=0)),
    ("2 d = rate", lambda c: dict(m=5, capacity=1, d=2, params=params_of(5, c["rounds"]))),
    ("2 d above the rate", lambda c: dict(d=3)),
    ("m = 3 never qualifies", lambda c: dict(m=3, capacity=1, d=1, params=params_of(3, c["rounds"]))),
    ("rounds = 0", lambda c: dict(rounds=0)),
    ("rounds = 28", lambda c: dict(rounds=28)),
    ("depth = 0", lambda c: dict(depth=0, indices=[0, 0])),
    ("depth = 64", lambda c: dict(depth=64, indices=[0, 0])),
    ("an index is 1 << depth", lambda c: dict(indices=[1, 1 << c["depth"]])),
    ("leaves NULL", lambda c: dict(null=("leaves",))),
    ("indices NULL", lambda c: dict(null=("indices",))),
    ("paths NULL", lambda c: dict(null=("paths",))),
    ("output NULL", lambda c: dict(null=("out",))),
    ("params NULL", lambda c: dict(null=("params",))),
    ("a matrix entry is p", lambda c: p_at(c, 1)),
    ("the last constant is p", lambda c: p_at(c, len(c["params"]) // 16 - 1)),
    # k alone is absurd; the arrays are the two-item ones, every word of them valid: only the byte count can refuse the call, and it
    # must do so before the arrays are looked at (they end after two items)
    ("byte counts wrap: k", lambda c: dict(k=1 << 58)),
    ("byte counts wrap: the output", lambda c: dict(k=1 << 54)),
]
REFUSAL_SAYS = {"byte counts wrap: k": "byte counts wrap", "byte counts wrap: the output": "byte counts wrap", "an index is 1 << depth": "invalid index",
                "2 d = rate": "2 * digest_len < rate", "2 d above the rate": "2 * digest_len < rate", "m = 3 never qualifies": "2 * digest_len < rate",
                "depth = 0": "depth of 1 .. 63", "depth = 64": "depth of 1 .. 63"}


def run_entry(c):
    rng = random.Random(9)
    words = lambda count: wc.pack([rng.randrange(P) for _ in range(count)])
    leaves, paths = words(2 * 4), words(2 * 4 * 64)
    idx = (ctypes.c_uint64 * len(c["indices"]))(*c["indices"])
    out = Window(2 * 12 * (3 * 28 + 1))
    null = c["null"]
    code = sc.lib().sc_rescue_merkle_path_trace_dev(None if "leaves" in null else leaves, None if "indices" in null else idx, None if "paths" in null else paths,
                                                    c["k"], c["depth"], c["d"], c["m"], c["m"] - c["capacity"], None if "params" in null else c["params"], c["rounds"],
                                                    None if "out" in null else out.ptr, None)
    sc.synchronize()
    out.read()
    return code, out.untouched


@pytest.mark.parametrize("name,change", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_write_nothing(name, change):
    c = good()
    c.update(change(c))
    code, untouched = run_entry(c)
    assert code == SC_ERR_BAD_ARG and untouched, (name, code)
    if name in REFUSAL_SAYS:
        assert REFUSAL_SAYS[name] in sc.lib().sc_last_error().decode(), (name, sc.lib().sc_last_error())


def test_the_call_the_refusals_start_from_is_taken_and_no_items_is_nothing():
    code, untouched = run_entry(good())
    assert code == SC_OK and not untouched, sc.lib().sc_last_error()
    c = good()
    c.update(k=0, null=("leaves", "indices", "paths", "out"))
    code, untouched = run_entry(c)
    assert code == SC_OK and untouched


# ---- the scheme -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def scheme(m, capacity, d, rounds, depth, s=2):
    tree = rescue_merkle.RescueMerkle(rescue_prime.RescuePrime(m=m, capacity=capacity, rounds=rounds), digest_len=d)
    return rescue_membership.RescueMembership(tree, depth, expansion_factor=4, num_colinearity_checks=s, security_level=2 * s)


@functools.lru_cache(maxsize=None)
def rows_of_tree(depth, seed=0):
    rng = random.Random(depth + 1000 * seed)
    return tuple(tuple(rng.randrange(P) for _ in range(3)) for _ in range(1 << depth))


def witness(sch, index, seed=0):
    rows = [list(r) for r in rows_of_tree(sch.depth, seed)]
    return sch.tree.commit(rows), sch.tree.leaf(rows[index]), sch.tree.open(index, rows)


HOST_FLOW, DEVICE_FLOW, WIDEST = (4, 1, 1, 3, 2), (4, 1, 1, 7, 3), (8, 3, 2, 27, 2)


def test_device_traces_equal_the_host_trace():
    sch = scheme(*DEVICE_FLOW)
    members = [witness(sch, i) for i in (0, 5, 7)]
    traces = sch.trace_batch_device([w[1] for w in members], [0, 5, 7], [w[2] for w in members])
    for trace, (root, leaf, path), index in zip(traces, members, (0, 5, 7)):
        want = sch.trace(leaf, index, path)
        assert isinstance(trace, DeviceTrace) and len(trace) == sch.T and len(trace.columns) == sch.W
        assert [sc.unpack(c.to_bytes()) for c in trace.columns] == [[row[s].value for row in want] for s in range(sch.W)]
        assert trace.entry(sch.T - 1, 0).value == root[0]
    places = [c.ptr for trace in traces for c in trace.columns]
    assert all(b - a == 16 * sch.T for a, b in zip(places, places[1:]))                    # views of one matrix: no copy
    one = sch.trace_device(members[1][1], 5, members[1][2])
    assert [c.to_bytes() for c in one.columns] == [c.to_bytes() for c in traces[1].columns]


@pytest.mark.parametrize("parameters,rows,device", [(HOST_FLOW, 17, False), (DEVICE_FLOW, 33, True), (WIDEST, 65, True)], ids=["host flow", "device flow", "m = 8, 27 rounds"])
def test_prove_and_verify(parameters, rows, device):
    sch = scheme(*parameters)
    assert sch.stark.randomized_trace_length == rows and sch._device_flow() is device and (rows >= FastStark.DEVICE_MIN) is device
    index = (1 << sch.depth) - 2
    root, leaf, path = witness(sch, index)
    proof = sch.prove(root, leaf, index, path)
    assert sch.verify(root, leaf, proof) is True
    if parameters == WIDEST:
        return
    assert sch.verify([(root[0] + 1) % P], leaf, proof) is False, "a wrong root"
    assert sch.verify(root, [(leaf[0] + 1) % P], proof) is False, "a wrong leaf digest"
    # another tree: other rows under the same hash, and the same rows under another hash
    other_root, other_leaf, other_path = witness(sch, index, seed=1)
    assert sch.verify(root, leaf, sch.prove(other_root, other_leaf, index, other_path)) is False, "a proof for another tree's root"
    m, capacity, d, rounds, depth = parameters
    other_hash = rescue_prime.RescuePrime(m=m, capacity=capacity, rounds=rounds, security_level=120)            # other round constants
    elsewhere = rescue_membership.RescueMembership(rescue_merkle.RescueMerkle(other_hash, digest_len=d), depth, 4, 2, 4)
    there = witness(elsewhere, index)
    assert there[0] != root and elsewhere.verify(there[0], there[1], elsewhere.prove(there[0], there[1], index, there[2])) is True
    assert sch.verify(there[0], there[1], elsewhere.prove(there[0], there[1], index, there[2])) is False, "a proof made over another hash"
    # false witnesses: the prover raises and returns nothing
    changed = [list(s) for s in path]
    changed[1][0] = (changed[1][0] + 1) % P
    with pytest.raises(AssertionError):
        sch.prove(root, leaf, index, changed)
    with pytest.raises(AssertionError):
        sch.prove(root, leaf, index ^ 1, path)


def test_prove_batch_is_three_proofs_byte_for_byte_and_verify_batch(seeded):
    sch = scheme(*DEVICE_FLOW)
    indices = [0, 3, 6]
    members = [witness(sch, i) for i in indices]
    roots, leaves, paths = [w[0] for w in members], [w[1] for w in members], [w[2] for w in members]
    seeded(0xBA7C4)
    one_by_one = [sch.prove(root, leaf, index, path) for root, leaf, index, path in zip(roots, leaves, indices, paths)]
    seeded(0xBA7C4)
    together = sch.prove_batch(roots, leaves, indices, paths)
    assert together == one_by_one and len(set(together)) == 3
    assert sch.prove_batch([], [], [], []) == [] and sch.verify_batch([], [], []) == []
    # a batch that mixes valid and tampered proofs, wrong statements among them
    broken = bytearray(together[1])
    broken[len(broken) // 2] ^= 1
    proofs = [together[0], bytes(broken), together[2], together[0], together[1], b"no proof"]
    said_roots = [roots[0], roots[1], [(roots[2][0] + 1) % P], roots[0], roots[1], roots[0]]
    said_leaves = [leaves[0], leaves[1], leaves[2], leaves[1], leaves[1], leaves[0]]

    def verdict(root, leaf, proof):
        try:
            return sch.verify(root, leaf, proof)
        except Exception:                              # noqa: BLE001  (verify_batch reports a proof on which verify raises as False)
            return False
    want = [verdict(*member) for member in zip(said_roots, said_leaves, proofs)]
    assert want == [True, False, False, False, True, False]
    assert sch.verify_batch(said_roots, said_leaves, proofs) == want
    with pytest.raises(AssertionError):
        sch.prove_batch(roots, leaves, [0, 2, 6], paths)


def test_a_batch_shares_one_air_launch(seeded, monkeypatch):
    """the prover extends its points by the public columns, so the constraints are ordinary value-domain work: the AIR of all
    constraints and members of a batch is one launch per value-domain order (the 2 m + 1 constraints have three degree bounds at the
    most: rounds, the bit and the swaps, the constants after a junction), and one proof evaluates no constraint symbolically"""
    sch = scheme(*DEVICE_FLOW)
    indices = [1, 4]
    members = [witness(sch, i) for i in indices]
    arguments = [w[0] for w in members], [w[1] for w in members], indices, [w[2] for w in members]
    seeded(77)
    want = [sch.prove(root, leaf, index, path) for root, leaf, index, path in zip(*arguments)]
    calls = {}
    real = sc.lib()

    class Counted:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if not name.startswith("sc_"):
                return fn

            def counted(*args):
                calls[name] = calls.get(name, 0) + 1
                return fn(*args)
            return counted
    monkeypatch.setattr(sc, "lib", lambda: Counted())
    seeded(77)
    got = sch.prove_batch(*arguments)
    batch_calls = dict(calls)
    calls.clear()
    seeded(77)
    alone = sch.prove(*[a[0] for a in arguments])
    monkeypatch.undo()
    assert got == want and alone == want[0]
    assert 1 <= batch_calls.get("sc_mpoly_eval_columns_dev", 0) <= 3 and "sc_mpoly_eval_dev" not in batch_calls and "sc_mpoly_eval_rot_dev" not in batch_calls
    assert calls.get("sc_mpoly_eval_rot_dev", 0) == 2 * sch.m + 1 and "sc_mpoly_eval_dev" not in calls


def test_prove_batch_on_the_host_flow_is_sequential(seeded):
    sch = scheme(*HOST_FLOW)
    members = [witness(sch, i) for i in (1, 2)]
    seeded(5)
    want = [sch.prove(w[0], w[1], i, w[2]) for w, i in zip(members, (1, 2))]
    seeded(5)
    assert sch.prove_batch([w[0] for w in members], [w[1] for w in members], [1, 2], [w[2] for w in members]) == want


def test_prove_rows_from_a_resident_tree():
    sch = scheme(*DEVICE_FLOW)
    rows = [list(r) for r in rows_of_tree(sch.depth)]
    n, width = len(rows), len(rows[0])
    matrix = sc.DeviceVector.from_bytes(sc.pack([row[j] for j in range(width) for row in rows]))
    resident = sch.tree.build_device(matrix, n, width)
    root, leaves, proofs = sch.prove_rows(resident, [6, 1], [rows[6], rows[1]])
    assert root == sch.tree.commit(rows) and leaves == [sch.tree.leaf(rows[6]), sch.tree.leaf(rows[1])] and len(proofs) == 2
    assert sch.verify_batch([root, root], leaves, proofs) == [True, True]
    assert sch.verify(root, leaves[0], proofs[1]) is False
    with pytest.raises(AssertionError):
        sch.prove_rows(resident, [6], [rows[5]])                                            # not the row at that leaf
    with pytest.raises(AssertionError, match="depth"):
        scheme(*HOST_FLOW).prove_rows(resident, [0], [rows[0]])


def test_existing_proofs_do_not_move(seeded):
    """the degree hook changes nothing for constraints with a dictionary: a reference proof of tests/golden/fast_stark.json and the
    reference's signature of tests/golden/rpsss.json come out byte for byte"""
    from fast_rpsss import FastRPSSS
    field, rp = Field.main(), rescue_prime.RescuePrime()
    rec = load_golden("fast_stark.json")["runs"][0]
    seeded(rec["urandom_seed"])
    input_element = FieldElement(int(rec["input"]), field)
    stark = FastStark(field, rec["expansion_factor"], rec["num_colinearity_checks"], rec["security_level"], rp.m, rp.N + 1)
    tz, tz_codeword, tz_root = stark.preprocess()
    air, boundary = rp.transition_constraints(stark.omicron), rp.boundary_constraints(rp.hash(input_element))
    assert all(getattr(a, "degree_bound", None) is None for a in air)
    proof = stark.prove(rp.trace(input_element), air, boundary, tz, tz_codeword)
    assert len(proof) == rec["proof_len"] and hashlib.sha256(proof).hexdigest() == rec["proof_sha256"]
    g = load_golden("rpsss.json")
    rpsss = FastRPSSS()
    seeded(g["seed"])
    pairs = [rpsss.keygen() for _ in range(len(g["keys"]))]
    signature = rpsss.sign(pairs[g["signed_key"]][0], g["document"].encode())
    assert len(signature) == g["signature_len"] and hashlib.sha256(signature).hexdigest() == g["signature_sha256"]
