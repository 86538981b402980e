"""The generic-width Rescue-Prime entries (sc_rescue_prime_permute_dev, _sponge_dev, _trace_states_dev; csrc/rescue.hip) and the
RescuePrime methods over them, on the cases of tests/rescue_wide_cases.py: every width 2 .. 8, the workgroup boundary, strided and
in place, 1 and 27 rounds, the edge words in every register position; the sponge over 1, 2 and 5 blocks; all states; every refusal;
a caller's stream; and a proof through FastStark at widths 3 (register by register) and 4 (column batches).

Every launch writes into a window of a larger vector filled with a sentinel residue; afterwards the window equals the plain-integer
model in every lane, the guards and the gaps between rows hold the sentinel and the input's bytes are what they were.  Exact."""
import ctypes
import random

import pytest

import rescue_wide_cases as wc

pytestmark = pytest.mark.gpu

import starkcore as sc                              # noqa: E402
import rescue_prime                                 # noqa: E402
from algebra import Field, FieldElement             # noqa: E402

P = wc.P
SC_OK, SC_ERR_BAD_ARG = 0, -6
GUARD = 64
SENTINEL_INT = random.Random(0x5E472).randrange(2, P - 1)     # a residue: no result is told apart from it by its range
SENTINEL = sc.fe_bytes(SENTINEL_INT)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert sc.device_count() > 0, "no GPU visible"
    sc.init()


class Window:
    """`elems` elements GUARD elements inside a vector of sentinels (or of `content`, for a call in place)"""

    def __init__(self, elems, content=None):
        self.elems = elems
        self.before = SENTINEL * GUARD + (SENTINEL * elems if content is None else content) + SENTINEL * GUARD
        self.vec = sc.DeviceVector.from_bytes(self.before)
        self.ptr = self.vec.ptr + 16 * GUARD

    def read(self):
        raw = self.vec.to_bytes()
        self.guards_hold = raw[:16 * GUARD] == SENTINEL * GUARD and raw[16 * (GUARD + self.elems):] == SENTINEL * GUARD
        self.untouched = raw == self.before
        return wc.unpack(raw[16 * GUARD:16 * (GUARD + self.elems)])


def rows_of(flat, height, n, ld):
    """(per input its `height` words, the words between n and ld of every row but the last)"""
    return [[flat[j * ld + k] for j in range(height)] for k in range(n)], [flat[j * ld + k] for j in range(height - 1) for k in range(n, ld)]


def permute(m, rounds, n, ld, in_place, stream=None):
    mds, rc = wc.seeded_params(m, rounds)
    states = [list(s) for s in wc.input_states(m)[:n]]
    matrix = wc.pack(wc.coalesced(states, n, ld, SENTINEL_INT))
    elems = (m - 1) * ld + n
    if in_place:
        out = Window(elems, matrix)
        src_ptr = out.ptr
    else:
        src, out = sc.DeviceVector.from_bytes(matrix), Window(elems)
        src_ptr = src.ptr
    if stream is not None:
        sc.synchronize()
    code = sc.lib().sc_rescue_prime_permute_dev(src_ptr, ld, out.ptr, ld, n, m, wc.params_bytes(mds, rc), rounds, stream)
    if stream is not None:
        import torch
        torch.cuda.synchronize()
    assert code == SC_OK, sc.lib().sc_last_error()
    got, gaps = rows_of(out.read(), m, n, ld)
    want = [list(st[rounds]) for st in wc.reference_states(m, rounds)[:n]]
    assert got == want, ("first lane that differs", next(k for k in range(n) if got[k] != want[k]))
    assert all(v == SENTINEL_INT for v in gaps) and out.guards_hold
    if not in_place:
        assert src.to_bytes() == matrix


@pytest.mark.parametrize("rounds", [1, 27])
@pytest.mark.parametrize("m", wc.WIDTHS)
def test_permute_equals_the_model(m, rounds):
    for n in (1, 255, 256, 257):
        for ld in (n, n + 3):
            for in_place in (False, True):
                permute(m, rounds, n, ld, in_place)


def sponge_call(m, rate, blocks, out_len, n, ld_msg, ld_out, msgs, params, rounds, stream=None):
    matrix = wc.pack(wc.coalesced([msg[:blocks * rate] for msg in msgs], n, ld_msg, SENTINEL_INT))
    src, out = sc.DeviceVector.from_bytes(matrix), Window((out_len - 1) * ld_out + n)
    code = sc.lib().sc_rescue_prime_sponge_dev(src.ptr, ld_msg, blocks, out.ptr, ld_out, out_len, n, m, rate, params, rounds, stream)
    sc.synchronize()
    assert code == SC_OK, sc.lib().sc_last_error()
    got, gaps = rows_of(out.read(), out_len, n, ld_out)
    assert all(v == SENTINEL_INT for v in gaps) and out.guards_hold and src.to_bytes() == matrix
    return got


@pytest.mark.parametrize("m,rate", wc.SPONGE_SHAPES)
def test_sponge_equals_the_model(m, rate):
    n, rounds = wc.SPONGE_N, wc.SPONGE_ROUNDS
    params = wc.params_bytes(*wc.seeded_params(m, rounds))
    msgs, after = [list(msg) for msg in wc.sponge_messages(m, rate)], wc.sponge_reference(m, rate)
    for blocks in wc.SPONGE_BLOCKS:
        for out_len in sorted({1, rate}):
            got = sponge_call(m, rate, blocks, out_len, n, n + 3, n + 1, msgs, params, rounds)
            assert got == [list(after[k][blocks - 1][:out_len]) for k in range(n)], (blocks, out_len)
    if (m, rate) == (2, 1):
        # one block: sc_rescue_prime_hash_dev on the same inputs, bit for bit
        xs = sc.DeviceVector.from_bytes(wc.pack([msg[0] for msg in msgs]))
        hashes = sc.DeviceVector(n)
        assert sc.lib().sc_rescue_prime_hash_dev(xs.ptr, n, params, rounds, hashes.ptr, None) == SC_OK
        got = sponge_call(2, 1, 1, 1, n, n, n, msgs, params, rounds)
        assert wc.pack([v for (v,) in got]) == hashes.to_bytes()


@pytest.mark.parametrize("m,capacity,rounds", [(3, 1, 7), (4, 2, 27), (8, 1, 3)])
def test_sponge_batch_and_compress_equal_the_host_sponge(m, capacity, rounds):
    rp = rescue_prime.RescuePrime(m=m, capacity=capacity, rounds=rounds)
    mds, rc = [v for row in rp._mds for v in row], rp._constants
    rng = random.Random(m)
    for length in (0, 1, rp.rate, 2 * rp.rate + 1):
        msgs = [[rng.randrange(P) for _ in range(length)] for _ in range(9)]
        for out_len in sorted({1, rp.rate}):
            got = rp.sponge_batch(msgs, out_len)
            assert got == [rp.sponge(msg, out_len) for msg in msgs]
            assert got == [wc.sponge(msg, m, rp.rate, mds, rc, rounds, out_len) for msg in msgs]
    left, right = [rng.randrange(P) for _ in range(70)], [FieldElement(rng.randrange(P), rp.field) for _ in range(70)]
    assert rp.compress(left, right) == [rp.sponge([a, b]) for a, b in zip(left, right)]
    states = [list(s) for s in wc.input_states(m)[:5]]
    out = rp.permutation_device(sc.DeviceVector.from_bytes(wc.pack(wc.coalesced(states, 5, 5, 0))), 5)
    assert rows_of(sc.unpack(out.to_bytes()), m, 5, 5)[0] == [rp.permutation(s) for s in states]
    xs = [FieldElement(v, rp.field) for v in left[:5]]
    assert rp.hash_batch(xs) == [rp.hash(x) for x in xs]
    with pytest.raises(AssertionError):
        rescue_prime.RescuePrime(m=2).compress([1], [2])              # rate 1 absorbs one element per permutation


@pytest.mark.parametrize("m", [2, 3, 4, 8])
def test_trace_states_equal_the_model(m):
    rounds = 27
    mds, rc = wc.seeded_params(m, rounds)
    params = wc.params_bytes(mds, rc)
    for n, ld in ((1, 1), (3, 5), (257, 257)):
        states = [list(s) for s in wc.input_states(m)[:n]]
        matrix = wc.pack(wc.coalesced(states, n, ld, SENTINEL_INT))
        src, out = sc.DeviceVector.from_bytes(matrix), Window(m * n * (rounds + 1))
        assert sc.lib().sc_rescue_prime_trace_states_dev(src.ptr, ld, n, m, params, rounds, out.ptr, None) == SC_OK, sc.lib().sc_last_error()
        sc.synchronize()
        assert out.read() == wc.expected_trace(m, rounds, n), n
        assert out.guards_hold and src.to_bytes() == matrix
    if m == 2:
        # the states (x, 0): sc_rescue_prime_trace_dev on the inputs x
        n = 257
        xs = [s[0] for s in wc.input_states(2)[:n]]
        old, new = sc.DeviceVector(2 * n * (rounds + 1)), sc.DeviceVector(2 * n * (rounds + 1))
        src = sc.DeviceVector.from_bytes(wc.pack(xs + [0] * n))
        assert sc.lib().sc_rescue_prime_trace_dev(src.ptr, n, params, rounds, old.ptr, None) == SC_OK
        assert sc.lib().sc_rescue_prime_trace_states_dev(src.ptr, n, n, 2, params, rounds, new.ptr, None) == SC_OK
        assert new.to_bytes() == old.to_bytes()


@pytest.mark.parametrize("m,capacity,rounds", [(2, 1, 27), (3, 1, 7), (4, 2, 7), (8, 4, 27)])
def test_trace_device_reads_back_equal_to_trace(m, capacity, rounds):
    rp = rescue_prime.RescuePrime(m=m, capacity=capacity, rounds=rounds)
    single = FieldElement(wc.input_states(m)[3][0] % P, rp.field)
    for inputs in (single, [single], [FieldElement(7 + s, rp.field) for s in range(rp.rate)]):
        trace = rp.trace_device(inputs)
        want = rp.trace(inputs)
        assert len(trace.columns) == m and len(trace) == rounds + 1
        assert [sc.unpack(c.to_bytes()) for c in trace.columns] == [[row[s].value for row in want] for s in range(m)]
        assert trace.entry(rounds, 0) == rp.hash(inputs)
    # many inputs: rate rows of n elements
    n = 3
    rows = [[FieldElement(100 * k + j, rp.field) for j in range(rp.rate)] for k in range(n)]
    whole = rp.trace_batch_device(sc.DeviceVector.from_bytes(wc.pack(wc.coalesced([[v.value for v in r] for r in rows], n, n, 0))), n)
    got = sc.unpack(whole.to_bytes())
    for k in range(n):
        want = rp.trace(rows[k])
        for s in range(m):
            assert got[(m * k + s) * (rounds + 1):(m * k + s + 1) * (rounds + 1)] == [row[s].value for row in want]


# ---- refusals -------------------------------------------------------------------------------------------------------------------

def good_call(m=4, rate=2, rounds=3, n=5, blocks=2, out_len=2):
    mds, rc = wc.seeded_params(m, rounds)
    return dict(m=m, rate=rate, rounds=rounds, n=n, blocks=blocks, out_len=out_len, ld_in=n + 1, ld_out=n + 2, params=wc.params_bytes(mds, rc),
                null_in=False, null_out=False, null_params=False, out_at=None)


def refusals():
    """(name, the entries it applies to, what to change in good_call)"""
    p_at = lambda index: lambda c: dict(params=c["params"][:16 * index] + sc.fe_bytes(P) + c["params"][16 * (index + 1):])
    last = lambda c: len(c["params"]) // 16 - 1
    return [
        ("m = 1", "pst", lambda c: dict(m=1)),
        ("m = 9", "pst", lambda c: dict(m=9)),
        ("m = 0", "pst", lambda c: dict(m=0)),
        ("rate = 0", "s", lambda c: dict(rate=0)),
        ("rate = m", "s", lambda c: dict(rate=c["m"])),
        ("out_len = 0", "s", lambda c: dict(out_len=0)),
        ("out_len = rate + 1", "s", lambda c: dict(out_len=c["rate"] + 1)),
        ("blocks = 0", "s", lambda c: dict(blocks=0)),
        ("rounds = 0", "pst", lambda c: dict(rounds=0)),
        ("rounds = 28", "pst", lambda c: dict(rounds=28)),
        ("a matrix entry is p", "pst", lambda c: p_at(1)(c)),
        ("the last constant is p", "pst", lambda c: p_at(last(c))(c)),
        ("the last constant is 2^128 - 1", "pst", lambda c: dict(params=c["params"][:-16] + sc.fe_bytes(wc.TOP))),
        ("params NULL", "pst", lambda c: dict(null_params=True)),
        ("input NULL", "pst", lambda c: dict(null_in=True)),
        ("output NULL", "pst", lambda c: dict(null_out=True)),
        ("input stride below n", "pst", lambda c: dict(ld_in=c["n"] - 1)),
        ("output stride below n", "ps", lambda c: dict(ld_out=c["n"] - 1)),
        ("output starts inside the input", "pst", lambda c: dict(out_at=16)),
        ("output ends inside the input", "pst", lambda c: dict(out_at=-16)),
        ("in place with another stride", "p", lambda c: dict(out_at=0, ld_out=c["ld_in"] + 1)),
        ("in place", "st", lambda c: dict(out_at=0, ld_out=c["ld_in"])),
    ]


def run_entry(entry, c):
    """one call of entry 'p', 's' or 't' with the arguments c; the input lies in a window too, so an output placed over it (out_at:
    a byte offset from the input's start) stays inside one vector.  Returns (code, input window, output window or None)."""
    m, n, rounds = max(1, min(c["m"], 8)), c["n"], max(1, min(c["rounds"], 27))
    in_rows = m if entry != "s" else max(1, c["blocks"]) * max(1, min(c["rate"], 8))
    out_elems = m * n * (rounds + 1) if entry == "t" else max(m, c["out_len"], 1) * max(c["ld_out"], n)
    rng = random.Random(5)
    content = wc.pack([rng.randrange(P) for _ in range(in_rows * max(c["ld_in"], n) + out_elems)])     # room for an output laid over it
    src = Window(len(content) // 16, content)
    out = None if c["out_at"] is not None else Window(out_elems)
    d_in = None if c["null_in"] else src.ptr
    d_out = None if c["null_out"] else (src.ptr + c["out_at"] if out is None else out.ptr)
    if c["out_at"] is not None and c["out_at"] < 0:
        d_in, d_out = src.ptr - c["out_at"], src.ptr
    params = None if c["null_params"] else c["params"]
    lib = sc.lib()
    if entry == "p":
        code = lib.sc_rescue_prime_permute_dev(d_in, c["ld_in"], d_out, c["ld_out"], n, c["m"], params, c["rounds"], None)
    elif entry == "s":
        code = lib.sc_rescue_prime_sponge_dev(d_in, c["ld_in"], c["blocks"], d_out, c["ld_out"], c["out_len"], n, c["m"], c["rate"], params, c["rounds"], None)
    else:
        code = lib.sc_rescue_prime_trace_states_dev(d_in, c["ld_in"], n, c["m"], params, c["rounds"], d_out, None)
    sc.synchronize()
    return code, src, out


@pytest.mark.parametrize("name,entries,change", refusals(), ids=[r[0] for r in refusals()])
def test_refusals_write_nothing(name, entries, change):
    for entry in entries:
        c = good_call()
        c.update(change(c))
        code, src, out = run_entry(entry, c)
        assert code == SC_ERR_BAD_ARG, (entry, name, code)
        src.read()
        assert src.untouched, (entry, name)
        if out is not None:
            out.read()
            assert out.untouched, (entry, name)


def test_the_call_the_refusals_start_from_is_taken_and_no_inputs_do_nothing():
    for entry in "pst":
        code, src, out = run_entry(entry, good_call())
        assert code == SC_OK, (entry, sc.lib().sc_last_error())
        out.read()
        assert not out.untouched and out.guards_hold
        c = good_call()
        c.update(n=0, ld_in=0, ld_out=0)
        code, src, out = run_entry(entry, c)
        assert code == SC_OK, (entry, sc.lib().sc_last_error())
        src.read(), out.read()
        assert src.untouched and out.untouched
        c.update(null_in=True, null_out=True)                          # no buffers are needed for no inputs
        assert run_entry(entry, c)[0] == SC_OK
    # permute in place with equal strides is the one overlap that is taken (test_permute_equals_the_model checks its result)
    c = good_call()
    c.update(out_at=0, ld_out=c["ld_in"])
    assert run_entry("p", c)[0] == SC_OK


def test_on_a_callers_stream():
    import torch
    stream = torch.cuda.Stream(device=torch.device("cuda", 0))
    handle = ctypes.c_void_p(stream.cuda_stream)
    for m in (3, 8):
        permute(m, 27, 257, 260, False, stream=handle)
        permute(m, 27, 257, 257, True, stream=handle)
    # the library's own stream handed over as a caller would hand over any stream
    permute(4, 1, 255, 255, False, stream=ctypes.c_void_p(sc.library_stream()))
    # sponge and trace states on the caller's stream: the same bytes as on the library's
    m, rate, rounds, n = 4, 2, 27, wc.SPONGE_N
    params = wc.params_bytes(*wc.seeded_params(m, rounds))
    msgs = [list(msg) for msg in wc.sponge_messages(m, rate)]
    matrix = sc.DeviceVector.from_bytes(wc.pack(wc.coalesced([msg[:2 * rate] for msg in msgs], n, n, 0)))
    outs = [sc.DeviceVector.zeros(rate * n) for _ in range(2)]
    traces = [sc.DeviceVector.zeros(m * n * (rounds + 1)) for _ in range(2)]
    sc.synchronize()
    for out, trace, st in zip(outs, traces, (None, handle)):
        assert sc.lib().sc_rescue_prime_sponge_dev(matrix.ptr, n, 2, out.ptr, n, rate, n, m, rate, params, rounds, st) == SC_OK
        assert sc.lib().sc_rescue_prime_trace_states_dev(matrix.ptr, n, n, m, params, rounds, trace.ptr, st) == SC_OK
    torch.cuda.synchronize()
    sc.synchronize()
    assert outs[0].to_bytes() == outs[1].to_bytes() == wc.pack(wc.coalesced([list(st[1][:rate]) for st in wc.sponge_reference(m, rate)], n, n, 0))
    assert traces[0].to_bytes() == traces[1].to_bytes()


# ---- end to end -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,capacity", [(3, 1), (4, 2)], ids=["per-register", "column-batches"])
def test_prove_and_verify_through_fast_stark(m, capacity):
    from fast_stark import FastStark
    assert FastStark.COLUMN_BATCH_MIN == 4                             # width 3 proves register by register, width 4 in column batches
    field = Field.main()
    rp = rescue_prime.RescuePrime(m=m, capacity=capacity, rounds=7)
    inputs = [FieldElement(31337 + s, field) for s in range(rp.rate)]
    output = rp.hash(inputs)
    stark = FastStark(field, 4, 2, 2, m, 8, transition_constraints_degree=3)
    tz, tz_codeword, tz_root = stark.preprocess()
    # FastStark, like the reference, interpolates one boundary polynomial per register and takes no register without a condition:
    # the rate registers that boundary_constraints leaves free (1 .. rate - 1) are pinned to their inputs, as public inputs
    known = [(0, s, inputs[s]) for s in range(1, rp.rate)]
    assert sorted({register for _, register, _ in rp.boundary_constraints(output) + known}) == list(range(m))
    air, boundary = rp.transition_constraints(stark.omicron), rp.boundary_constraints(output) + known
    trace = rp.trace_device(inputs)
    assert trace.entry(7, 0) == output
    proof = stark.prove(trace, air, boundary, tz, tz_codeword)
    assert stark.verify(proof, air, boundary, tz_root) is True
    assert stark.verify(proof, air, rp.boundary_constraints(output + field.one()) + known, tz_root) is False
