"""The Rescue-Prime Merkle tree on the GPU (sc_rescue_merkle_*; csrc/rescue_merkle.hip and rescue_merkle.cuh) and
rescue_merkle.RescueMerkle over it, on the cases of tests/rescue_merkle_cases.py: every level of every tree against the
plain-integer model with the tuning key at 0 (one lane per node), 2^40 (one lane per state register) and 8 (mixed); openings;
batched verification in both forms; every refusal; callers' streams.

Results land in windows of larger buffers filled with a sentinel; afterwards the window equals the model, the guards hold the
sentinel and the inputs' bytes are what they were.  Exact."""
import ctypes
import random

import pytest

import rescue_merkle_cases as mc
import rescue_wide_cases as wc

pytestmark = pytest.mark.gpu

import starkcore as sc                              # noqa: E402
import rescue_prime                                 # noqa: E402
import rescue_merkle                                # noqa: E402

P = mc.P
SC_OK, SC_ERR_BAD_ARG = 0, -6
GUARD = 64
SENTINEL_INT = random.Random(0x5E472).randrange(2, P - 1)
SENTINEL = sc.fe_bytes(SENTINEL_INT)
ROUNDS = mc.SWEEP_ROUNDS
UNTOUCHED = 0x5A5A5A5A5A5A5A58                       # what *tree holds before a call that must leave it alone


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert sc.device_count() > 0, "no GPU visible"
    sc.init()


@pytest.fixture(autouse=True)
def _restore_key():
    yield
    rescue_merkle.set_split_max_nodes(-1)


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


class HostWindow:
    """`nbytes` bytes 64 bytes inside a host buffer of 0xA5"""

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.buf = ctypes.create_string_buffer(b"\xA5" * (nbytes + 128), nbytes + 128)
        self.ptr = ctypes.c_void_p(ctypes.addressof(self.buf) + 64)

    def read(self):
        raw = self.buf.raw
        self.guards_hold = raw[:64] == b"\xA5" * 64 and raw[64 + self.nbytes:] == b"\xA5" * 64
        self.untouched = raw == b"\xA5" * (self.nbytes + 128)
        return raw[64:64 + self.nbytes]


def params_of(m, rounds):
    return wc.params_bytes(*wc.seeded_params(m, rounds))


class Built:
    """a tree built through the C entry over mc.rows(m, n, width) at stride ld"""

    def __init__(self, m, capacity, d, n, width, ld, rounds=ROUNDS, stream=None):
        self.m, self.d, self.n, self.rate, self.width, self.rounds = m, d, n, m - capacity, width, rounds
        self.rows = [list(r) for r in mc.rows(m, n, width)]
        self.matrix = wc.pack(wc.coalesced(self.rows, n, ld, SENTINEL_INT))
        self.src = sc.DeviceVector.from_bytes(self.matrix)
        self.h = ctypes.c_void_p()
        if stream is not None:
            sc.synchronize()
        code = sc.lib().sc_rescue_merkle_build_dev(self.src.ptr, ld, width, n, d, m, self.rate, params_of(m, rounds), rounds, ctypes.byref(self.h), stream)
        assert code == SC_OK, sc.lib().sc_last_error()
        assert sc.lib().sc_rescue_merkle_leaves(self.h) == n

    def levels(self, stream=None):
        """every level through level_copy, one behind the other in one guarded window"""
        out, at, shapes = Window(self.d * (2 * self.n - 1)), 0, []
        for j in range(self.n.bit_length()):
            assert sc.lib().sc_rescue_merkle_level_copy_dev(self.h, j, out.ptr + 16 * at, stream) == SC_OK, sc.lib().sc_last_error()
            shapes.append((at, self.n >> j))
            at += self.d * (self.n >> j)
        if stream is not None:
            import torch
            torch.cuda.synchronize()
        words = out.read()
        assert out.guards_hold and self.src.to_bytes() == self.matrix
        return [[[words[at + e * w + k] for e in range(self.d)] for k in range(w)] for at, w in shapes]

    def root(self):
        out = HostWindow(16 * self.d)
        assert sc.lib().sc_rescue_merkle_root(self.h, out.ptr) == SC_OK, sc.lib().sc_last_error()
        raw = out.read()
        assert out.guards_hold
        return wc.unpack(raw)

    def open_batch(self, indices):
        k, depth = len(indices), self.n.bit_length() - 1
        out = HostWindow(16 * self.d * depth * k)
        idx = (ctypes.c_uint64 * max(k, 1))(*indices)
        assert sc.lib().sc_rescue_merkle_open_batch(self.h, idx, k, out.ptr) == SC_OK, sc.lib().sc_last_error()
        words = wc.unpack(out.read())
        assert out.guards_hold and list(idx[:k]) == list(indices)
        return [[words[(t * depth + j) * self.d:(t * depth + j + 1) * self.d] for j in range(depth)] for t in range(k)]

    def free(self):
        assert sc.lib().sc_rescue_merkle_free(self.h) == SC_OK
        self.h = None


def as_lists(levels):
    return [[list(dg) for dg in level] for level in levels]


@pytest.mark.parametrize("m,capacity,d", mc.SHAPES)
def test_every_level_equals_the_model(m, capacity, d):
    rate = m - capacity
    assert mc.node_blocks(rate, d) == {(3, 1, 1): 2, (4, 1, 1): 1, (4, 2, 2): 3, (8, 3, 2): 1}.get((m, capacity, d), 1)
    for n, width in mc.tree_cases(rate) + ([mc.DEEP_CASE] if (m, capacity, d) == mc.DEEP_SHAPE else []):
        want = as_lists(mc.reference(m, capacity, d, n, width, ROUNDS))
        for key in mc.KEYS:
            rescue_merkle.set_split_max_nodes(key)
            for ld in (n, n + 3):
                tree = Built(m, capacity, d, n, width, ld)
                got = tree.levels()
                assert len(got) == len(want)
                for j, (g, w) in enumerate(zip(got, want)):
                    assert g == w, (n, width, key, ld, "level", j, "first node that differs", next(k for k in range(len(w)) if g[k] != w[k]))
                assert tree.root() == want[-1][0]
                tree.free()


@pytest.mark.parametrize("m", range(3, 9))
def test_full_rounds(m):
    n, rate, rounds = 64, m - 1, 27
    mds, rc = wc.seeded_params(m, rounds)
    rows = [list(r) for r in mc.rows(m, n, rate + 1)]
    want = mc.build(rows, m, rate, 1, mds, rc, rounds)
    rescue_merkle.set_split_max_nodes(8)
    tree = Built(m, 1, 1, n, rate + 1, n + 3, rounds=rounds)
    assert tree.levels() == want
    tree.free()


@pytest.mark.parametrize("m,capacity,d", [(4, 2, 2), (7, 1, 1)])
def test_open_batch(m, capacity, d):
    rate = m - capacity
    for n, width in ((256, rate + 1), (2, 1), (1, 1)):
        want = as_lists(mc.reference(m, capacity, d, n, width, ROUNDS))
        tree = Built(m, capacity, d, n, width, n)
        for indices in ([n // 2], [(0, n - 1, n // 2, n - 1)[t % 4] for t in range(65)], []):
            assert tree.open_batch(indices) == [mc.path(want, i) for i in indices]
        tree.free()


def verify_call(m, capacity, d, items, depth, key, rounds=ROUNDS):
    """items: (root, index, path, row) -> the verdict bytes, written into a guarded host window"""
    k, width = len(items), len(items[0][3])
    roots = wc.pack([v for it in items for v in it[0]])
    paths = wc.pack([v for it in items for s in it[2] for v in s])
    rows = wc.pack([v for it in items for v in it[3]])
    idx = (ctypes.c_uint64 * k)(*[it[1] for it in items])
    out = HostWindow(k)
    rescue_merkle.set_split_max_nodes(key)
    code = sc.lib().sc_rescue_merkle_verify_batch(roots, idx, paths if depth else None, rows, k, depth, width, d, m, m - capacity, params_of(m, rounds), rounds, out.ptr)
    assert code == SC_OK, sc.lib().sc_last_error()
    got = list(out.read())
    assert out.guards_hold
    return got


@pytest.mark.parametrize("m,capacity,d", [(3, 1, 1), (4, 2, 2), (7, 1, 1), (8, 3, 2)])
def test_verify_batch(m, capacity, d):
    rate = m - capacity
    mds, rc = wc.seeded_params(m, ROUNDS)
    for n, width in ((mc.DEEP_CASE if (m, capacity, d) == mc.DEEP_SHAPE else (2048, 1)), (1, rate + 1)):
        depth = n.bit_length() - 1
        levels = as_lists(mc.reference(m, capacity, d, n, width, ROUNDS))
        rows, root = [list(r) for r in mc.rows(m, n, width)], levels[-1][0]
        rng = random.Random(m + depth)
        for k in (1, 63, 64, 65):
            picks = [rng.randrange(n) for _ in range(k)]
            valid = [(root, i, mc.path(levels, i), rows[i]) for i in picks]
            mixed, want = [], []
            for t, item in enumerate(valid):
                changes = mc.tampered(*item, depth, d)
                if t % 2:
                    mixed.append(changes[(t // 2) % len(changes)][1:])
                else:
                    mixed.append(item)
                want.append(1 - t % 2)
            if k == 65:                     # the model agrees on which items a change has spoilt
                assert [int(mc.verify(*it, m, rate, d, mds, rc, ROUNDS)) for it in mixed[:6]] == want[:6]
            for key in (0, 1 << 40):
                assert verify_call(m, capacity, d, valid, depth, key) == [1] * k, (n, k, key)
                assert verify_call(m, capacity, d, mixed, depth, key) == want, (n, k, key)


def test_every_single_change_is_caught():
    m, capacity, d, n, width = 4, 2, 2, 2048, 1
    levels = as_lists(mc.reference(m, capacity, d, n, width, ROUNDS))
    rows, index = mc.rows(m, n, width), 1365
    item = (levels[-1][0], index, mc.path(levels, index), list(rows[index]))
    changes = mc.tampered(*item, 11, d)
    assert len(changes) == d + 11 + 1 + 11
    for key in (0, 1 << 40):
        assert verify_call(m, capacity, d, [item] + [c[1:] for c in changes], 11, key) == [1] + [0] * len(changes)


def test_python_class_and_the_fold_of_compress():
    rp = rescue_prime.RescuePrime(m=4, capacity=1, rounds=2)
    tree = rescue_merkle.RescueMerkle(rp)
    rows = [[(5 * i + j) * 0x123456789ABCDEF % P for j in range(4)] for i in range(8)]
    built = tree._rows_device(rows)
    assert built.leaves == 8 and built.depth == 3
    level = [dg[0] for dg in built.level(0)]
    assert level == [tree.leaf(r)[0] for r in rows]
    while len(level) > 1:
        level = [dg[0] for dg in rp.compress(level[0::2], level[1::2])]
    assert built.root() == level == tree.commit(rows) == tree.commit_rows(rows)
    matrix = sc.DeviceVector.from_bytes(sc.pack([row[j] for j in range(4) for row in rows]))
    assert tree.commit_device(matrix, 8, 4) == level
    assert built.level(3) == [level] and built.open(5) == tree.open(5, rows)
    paths = tree.open_rows([0, 7, 7], rows)
    assert paths == [tree.open(i, rows) for i in (0, 7, 7)]
    roots = [tree.commit(rows)] * 3
    assert tree.verify_batch(roots, [0, 7, 7], paths, [rows[0], rows[7], rows[6]]) == [True, True, False]
    assert tree.verify_batch([], [], [], []) == []
    wide = rescue_merkle.RescueMerkle(rescue_prime.RescuePrime(m=8, capacity=3, rounds=2), digest_len=2)
    assert wide.commit_rows(rows) == wide.commit(rows) and wide.open_rows([3], rows) == [wide.open(3, rows)]
    with pytest.raises(AssertionError, match="cannot open invalid index"):
        built.open(8)
    with pytest.raises(AssertionError, match="length must be power of two"):
        tree.commit_rows(rows[:3])


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def good():
    m, rate, rounds = 4, 3, 2
    return dict(m=m, rate=rate, d=2, rounds=rounds, width=3, n=8, ld=9, depth=3, level=1, params=params_of(m, rounds), k=2, indices=[1, 7],
                null=())


def p_at(c, word):
    return dict(params=c["params"][:16 * word] + sc.fe_bytes(P) + c["params"][16 * (word + 1):])


REFUSALS = [
    ("m = 1", "bv", lambda c: dict(m=1)),
    ("m = 9", "bv", lambda c: dict(m=9)),
    ("rate = 1", "bv", lambda c: dict(rate=1)),
    ("rate = m", "bv", lambda c: dict(rate=c["m"])),
    ("digest_len = 0", "bv", lambda c: dict(d=0)),
    ("digest_len = rate + 1", "bv", lambda c: dict(d=c["rate"] + 1)),
    ("rounds = 0", "bv", lambda c: dict(rounds=0)),
    ("rounds = 28", "bv", lambda c: dict(rounds=28)),
    ("width = 0", "bv", lambda c: dict(width=0)),
    ("N = 0", "b", lambda c: dict(n=0)),
    ("N = 6", "b", lambda c: dict(n=6)),
    ("ld below N", "b", lambda c: dict(ld=c["n"] - 1)),
    ("rows NULL", "bv", lambda c: dict(null=("rows",))),
    ("tree NULL", "bolr", lambda c: dict(null=("tree",))),
    ("params NULL", "bv", lambda c: dict(null=("params",))),
    ("output NULL", "olvr", lambda c: dict(null=("out",))),
    ("indices NULL", "ov", lambda c: dict(null=("indices",))),
    ("roots NULL", "v", lambda c: dict(null=("roots",))),
    ("paths NULL", "v", lambda c: dict(null=("paths",))),
    ("a matrix entry is p", "bv", lambda c: p_at(c, 1)),
    ("the last constant is p", "bv", lambda c: p_at(c, len(c["params"]) // 16 - 1)),
    ("an index is N", "o", lambda c: dict(indices=[1, c["n"]])),
    ("an index is 1 << depth", "v", lambda c: dict(indices=[1, 1 << c["depth"]])),
    ("depth = 64", "v", lambda c: dict(depth=64, indices=[0, 0])),
    ("level above log2 N", "l", lambda c: dict(level=4)),
    ("byte counts wrap: width", "b", lambda c: dict(width=1 << 61, ld=1 << 62, n=8)),
    ("byte counts wrap: N", "b", lambda c: dict(n=1 << 62, ld=1 << 62)),
    # k alone is absurd; the arrays are the two-item ones of the call that is taken, and every word of them is a valid index, so
    # only the byte count can refuse the call -- and it must do so before the arrays are looked at (they end after two items)
    ("byte counts wrap: k", "ov", lambda c: dict(k=1 << 62, indices=[1, 7])),
    ("byte counts wrap: k * width", "v", lambda c: dict(k=1 << 40, width=1 << 40, indices=[1, 7])),
]
# what sc_last_error must say for the refusals that several checks could give
REFUSAL_SAYS = {"byte counts wrap: width": "byte counts wrap", "byte counts wrap: N": "byte counts wrap", "byte counts wrap: k": "byte counts wrap",
                "byte counts wrap: k * width": "byte counts wrap", "an index is N": "invalid index", "an index is 1 << depth": "invalid index"}


def run_entry(entry, c, tree):
    """one call of build ('b'), open_batch ('o'), level_copy ('l'), root ('r') or verify_batch ('v'); returns (code, what must be untouched)"""
    lib, null = sc.lib(), c["null"]
    rng = random.Random(9)
    params = None if "params" in null else c["params"]
    if entry == "b":
        elems = 64
        src = Window(elems)
        holder = ctypes.c_void_p(UNTOUCHED)
        code = lib.sc_rescue_merkle_build_dev(None if "rows" in null else src.ptr, c["ld"], c["width"], c["n"], c["d"], c["m"], c["rate"], params,
                                              c["rounds"], None if "tree" in null else ctypes.byref(holder), None)
        sc.synchronize()
        src.read()
        return code, [src.untouched, holder.value == UNTOUCHED]
    if entry == "o":
        out = HostWindow(16 * 2 * 3 * len(c["indices"]))
        idx = (ctypes.c_uint64 * len(c["indices"]))(*c["indices"])
        code = lib.sc_rescue_merkle_open_batch(None if "tree" in null else tree.h, None if "indices" in null else idx, c["k"], None if "out" in null else out.ptr)
        out.read()
        return code, [out.untouched]
    if entry == "l":
        out = Window(64)
        code = lib.sc_rescue_merkle_level_copy_dev(None if "tree" in null else tree.h, c["level"], None if "out" in null else out.ptr, None)
        sc.synchronize()
        out.read()
        return code, [out.untouched]
    if entry == "r":
        out = HostWindow(32)
        code = lib.sc_rescue_merkle_root(None if "tree" in null else tree.h, None if "out" in null else out.ptr)
        out.read()
        return code, [out.untouched]
    k = len(c["indices"])
    words = lambda count: wc.pack([rng.randrange(P) for _ in range(count)])
    roots, paths, rows = words(k * 8), words(k * 8 * 3), words(k * 8)
    idx = (ctypes.c_uint64 * k)(*c["indices"])
    out = HostWindow(k)
    code = lib.sc_rescue_merkle_verify_batch(None if "roots" in null else roots, None if "indices" in null else idx, None if "paths" in null else paths,
                                             None if "rows" in null else rows, c["k"], c["depth"], c["width"], c["d"], c["m"], c["rate"], params,
                                             c["rounds"], None if "out" in null else out.ptr)
    out.read()
    return code, [out.untouched]


@pytest.fixture(scope="module")
def small_tree():
    tree = Built(4, 1, 2, 8, 3, 9)
    yield tree
    tree.free()


@pytest.mark.parametrize("name,entries,change", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_write_nothing(small_tree, name, entries, change):
    for entry in entries:
        c = good()
        c.update(change(c))
        code, untouched = run_entry(entry, c, small_tree)
        assert code == SC_ERR_BAD_ARG, (entry, name, code)
        assert all(untouched), (entry, name)
        if name in REFUSAL_SAYS:
            assert REFUSAL_SAYS[name] in sc.lib().sc_last_error().decode(), (entry, name, sc.lib().sc_last_error())


def test_the_calls_the_refusals_start_from_are_taken(small_tree):
    want = small_tree.levels()
    for entry in "bolrv":
        c = good()
        holder_before = None
        if entry == "b":
            # the good build call writes a tree: free it
            src = Window(64)
            h = ctypes.c_void_p(UNTOUCHED)
            assert sc.lib().sc_rescue_merkle_build_dev(src.ptr, c["ld"], c["width"], c["n"], c["d"], c["m"], c["rate"], c["params"], c["rounds"], ctypes.byref(h), None) == SC_OK
            assert h.value != UNTOUCHED and sc.lib().sc_rescue_merkle_free(h) == SC_OK
            continue
        code, untouched = run_entry(entry, c, small_tree)
        assert code == SC_OK, (entry, sc.lib().sc_last_error())
        assert not all(untouched), entry
    # nothing to do: no items, no openings
    c = good()
    c.update(k=0, indices=[], null=("roots", "paths", "rows", "out", "indices"))
    c["indices"] = [0]
    for entry in "ov":
        code, untouched = run_entry(entry, c, small_tree)
        assert code == SC_OK and all(untouched), entry
    assert small_tree.levels() == want


# ---- streams ----------------------------------------------------------------------------------------------------------------------

def test_on_a_callers_stream():
    import torch
    stream = torch.cuda.Stream(device=torch.device("cuda", 0))
    handle = ctypes.c_void_p(stream.cuda_stream)
    m, capacity, d, n, width = 4, 2, 2, 256, 3
    want = as_lists(mc.reference(m, capacity, d, n, width, ROUNDS))
    for key in mc.KEYS:
        rescue_merkle.set_split_max_nodes(key)
        tree = Built(m, capacity, d, n, width, n + 3, stream=handle)
        assert tree.levels(stream=handle) == want
        assert tree.open_batch([0, 255, 77]) == [mc.path(want, i) for i in (0, 255, 77)]
        assert tree.root() == want[-1][0]
        tree.free()


def test_two_builds_in_flight_on_two_streams():
    import torch
    streams = [torch.cuda.Stream(device=torch.device("cuda", 0)) for _ in range(2)]
    handles = [ctypes.c_void_p(s.cuda_stream) for s in streams]
    shapes = [(4, 2, 2, 256, 3), (7, 1, 1, 256, 7)]
    for key in (0, 1 << 40):
        rescue_merkle.set_split_max_nodes(key)
        single = []
        for shape in shapes:
            tree = Built(*shape, shape[3])
            single.append(tree.levels())
            tree.free()
        trees = [Built(*shape, shape[3], stream=h) for shape, h in zip(shapes, handles)]          # both enqueued before either is read
        got = [tree.levels(stream=h) for tree, h in zip(trees, handles)]
        assert got == single
        assert got == [as_lists(mc.reference(*shape, ROUNDS)) for shape in shapes]
        for tree in trees:
            tree.free()
