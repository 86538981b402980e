"""The Rescue-Prime kernels (sc_rescue_prime_hash_dev / sc_rescue_prime_trace_dev, csrc/rescue.hip) on the cases of
tests/rescue_prime_cases.py: lanes steered through 0, 1, p - 1 and residues with special Montgomery forms in front of every cube and
inverse cube, 1 to 27 rounds, the reference's, identity, zero, all-(p-1) and a random matrix, inputs at the reduction boundary,
elements of small and two-power order.  tests/test_rescue_prime_cases_cpu.py proves on the host that the cases reach those states.

Every launch writes into a window of a larger vector filled with a sentinel residue; afterwards the window equals the plain-integer
model in every lane, both guards hold the sentinel and the input's bytes are what they were.  Everything is exact."""
import ctypes
import random

import pytest

import rescue_prime_cases as rc

pytestmark = pytest.mark.gpu

import starkcore as sc                              # noqa: E402
import rescue_prime                                 # noqa: E402

P = rc.P
SC_OK, SC_ERR_BAD_ARG = 0, -6
GUARD = 64
SENTINEL = sc.fe_bytes(random.Random(0x5E471).randrange(2, P - 1))     # a residue: no result is told apart from it by its range
ENTRIES = ("sc_rescue_prime_hash_dev", "sc_rescue_prime_trace_dev")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert sc.device_count() > 0, "no GPU visible"
    sc.init()


def out_elems(entry, n, rounds):
    return n if entry == ENTRIES[0] else 2 * n * (rounds + 1)


class Launch:
    """Both entries on one case's inputs with the given parameter block, each into a window GUARD elements inside a vector of
    sentinels.  `stream`: a torch stream of the caller's, or None for the library's."""

    def __init__(self, case, params=None, rounds=None, stream=None):
        self.case = case
        self.rounds = case.rounds if rounds is None else rounds
        params = case.params if params is None else params
        self.src = sc.DeviceVector.from_bytes(case.input_bytes)
        # sized by the larger of the case's rounds and the call's: a call that should have been refused still writes inside the vector
        self.elems = [out_elems(e, case.n, max(case.rounds, self.rounds)) for e in ENTRIES]
        self.outs = [sc.DeviceVector.from_bytes(SENTINEL * (k + 2 * GUARD)) for k in self.elems]
        handle = None
        if stream is not None:
            sc.synchronize()                        # the uploads above are on the library's stream
            handle = ctypes.c_void_p(stream.cuda_stream)
        lib = sc.lib()
        self.codes = [getattr(lib, e)(self.src.ptr, case.n, params, self.rounds, out.ptr + 16 * GUARD, handle) for e, out in zip(ENTRIES, self.outs)]
        if stream is not None:
            import torch
            torch.cuda.synchronize()
        sc.synchronize()
        self.raw = [out.to_bytes() for out in self.outs]
        self.input_after = self.src.to_bytes()

    def windows(self):
        return [raw[16 * GUARD:16 * (GUARD + k)] for raw, k in zip(self.raw, self.elems)]

    def guards_hold(self):
        return all(raw[:16 * GUARD] == SENTINEL * GUARD and raw[16 * (GUARD + k):] == SENTINEL * GUARD for raw, k in zip(self.raw, self.elems))

    def untouched(self):
        return all(raw == SENTINEL * (k + 2 * GUARD) for raw, k in zip(self.raw, self.elems))


def first_difference(got, want):
    """(element index, got, want) of the first element that differs, for the assertion's message"""
    g, w = rc.unpack(got), rc.unpack(want)
    for i, (a, b) in enumerate(zip(g, w)):
        if a != b:
            return i, a, b
    return (min(len(g), len(w)), None, None) if len(g) != len(w) else None


def check(launch):
    case = launch.case
    assert launch.codes == [SC_OK, SC_OK], sc.lib().sc_last_error()      # the word behind the constants is not a residue and is not read
    got_hash, got_trace = launch.windows()
    assert got_hash == case.hash, ("hash (lane, got, want)", first_difference(got_hash, case.hash))
    rows = case.rounds + 1
    diff = first_difference(got_trace, case.trace)
    assert got_trace == case.trace, ("trace (lane, register, row), got, want", (diff[0] // (2 * rows), diff[0] // rows % 2, diff[0] % rows), diff[1:])
    assert launch.guards_hold()
    assert launch.input_after == case.input_bytes


@pytest.mark.parametrize("case", rc.ALL_CASES, ids=lambda c: c.name)
def test_steered_case_equals_the_model(case):
    check(Launch(case))


def test_structured_inputs_equal_the_model():
    case = rc.StructuredInputs
    check(Launch(case))
    rp = rescue_prime.RescuePrime()
    assert rp._params == case.params[:-16]
    vec = sc.DeviceVector.from_bytes(case.input_bytes)
    assert rp.hash_device(vec).to_bytes() == case.hash
    assert rp.trace_batch_device(vec).to_bytes() == case.trace
    assert vec.to_bytes() == case.input_bytes


def test_cases_on_a_callers_stream():
    """the same launches on a stream of the caller's: the same bytes as on the library's stream, guards included"""
    import torch
    stream = torch.cuda.Stream(device=torch.device("cuda", 0))
    for case in rc.STREAM_CASES:
        on_library = Launch(case)
        on_caller = Launch(case, stream=stream)
        check(on_caller)
        assert on_caller.raw == on_library.raw, case
    # the library's own stream, handed over as a caller would hand over any stream
    case = rc.STREAM_CASES[0]
    mine = Launch(case)
    lib, handle = sc.lib(), ctypes.c_void_p(sc.library_stream())
    outs = [sc.DeviceVector.from_bytes(SENTINEL * (k + 2 * GUARD)) for k in mine.elems]
    for entry, out in zip(ENTRIES, outs):
        assert getattr(lib, entry)(mine.src.ptr, case.n, case.params, case.rounds, out.ptr + 16 * GUARD, handle) == SC_OK
    sc.synchronize()
    assert [out.to_bytes() for out in outs] == mine.raw


@pytest.mark.parametrize("case", [rc.CASES[25], rc.CASES[7], rc.CASES[0]], ids=lambda c: c.name)
def test_refused_blocks_write_nothing(case):
    """a constant that is p -- the last one read, or a matrix entry -- and 28 rounds: SC_ERR_BAD_ARG, and neither window is written"""
    for what, params, rounds in rc.refused_blocks(case):
        launch = Launch(case, params=params, rounds=rounds)
        assert launch.codes == [SC_ERR_BAD_ARG, SC_ERR_BAD_ARG], what
        assert launch.untouched(), what
        assert launch.input_after == case.input_bytes, what
    # the same block with the word back in place is taken: the refusals above were about that word
    check(Launch(case))
