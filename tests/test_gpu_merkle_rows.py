"""Row commitments on the GPU (csrc/merkle_rows.cuh, csrc/merkle_rows.hip): sc_merkle_rows_build_dev / _async_dev /
_query_dev against the hashlib model of tests/merkle_rows_cases.py -- every width class of the block walk, every size at which the
build takes another path (below the fused entry, the first fused size, both sides of the tail kernel's width and of FUSE_MAX_W),
every level of the tree, values and paths into sentinel-guarded buffers, columns as views at odd offsets and as allocations of their
own, the refusals, two streams.  FastStark / FastRPSSS with row_commitments=True: tests/test_gpu_row_commitment_proofs.py."""
import ctypes
import random

import pytest

import merkle_rows_cases as cases

pytestmark = pytest.mark.gpu
vp, u64 = ctypes.c_void_p, ctypes.c_uint64
GUARD = b"\xEE"
SC_ERR_NOT_POW2, SC_ERR_BAD_ARG = -2, -6          # include/starkcore.h
WIDTHS = (1, 2, 7, 8, 9, 15, 16, 17, 24, 25, 128, 256)
SIZES = (1, 2, 4, 128, 256, 512, 2048, 4096, 1 << 17, 1 << 18)


@pytest.fixture(scope="module")
def sc():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible: the HIP path is mandatory for these tests"
    starkcore.init()
    return starkcore


# ---- helpers ---------------------------------------------------------------------------------------------------------------------------
def guarded(nbytes):
    """a host buffer of exactly nbytes sentinel bytes"""
    return ctypes.create_string_buffer(GUARD * nbytes, nbytes)


def resident(sc, packed_columns, layout):
    """the columns in HBM: (what keeps them alive, their device pointers) -- allocations of their own, or views at ODD element offsets
    into one allocation whose gaps hold a pattern no tree may pick up"""
    n, w = len(packed_columns[0]) // 16, len(packed_columns)
    if layout == "separate":
        vectors = [sc.DeviceVector.from_bytes(column) for column in packed_columns]
        return vectors, [v.ptr for v in vectors]
    pitch = n + 2 if n % 2 == 0 else n + 1          # even, so that every column starts at an odd element
    blob = bytearray(b"\xA5" * (16 * (1 + w * pitch)))
    for c, column in enumerate(packed_columns):
        blob[16 * (1 + c * pitch):16 * (1 + c * pitch + n)] = column
    vector = sc.DeviceVector.from_bytes(bytes(blob))
    return vector, [vector.ptr + 16 * (1 + c * pitch) for c in range(w)]


def build(sc, pointers, n, how="sync", stream=None):
    """-> MerkleTree over the handle (root fetched); the root buffer is guarded"""
    w = len(pointers)
    table, handle = (vp * w)(*pointers), vp()
    if how == "sync":
        root = guarded(128)
        sc._check(sc.lib().sc_merkle_rows_build_dev(table, w, n, root, ctypes.byref(handle), stream))
        assert root.raw[64:] == GUARD * 64
        return sc.MerkleTree(handle, root.raw[:64], n)
    sc._check(sc.lib().sc_merkle_rows_build_async_dev(table, w, n, ctypes.byref(handle), stream))
    return sc.MerkleTree(handle, None, n)


def query(sc, tree, pointers, indices, pinned=False):
    """sc_merkle_rows_query_dev into guarded buffers -> (rows bytes, paths bytes); pinned: one buffer of sc_host_alloc, which the
    kernel writes itself"""
    w, k, depth = len(pointers), len(indices), tree.depth
    row_bytes, path_bytes = 16 * k * w, 64 * depth * k
    table, idx = (vp * w)(*pointers), (u64 * max(k, 1))(*indices)
    if pinned:
        split = (row_bytes + 64 + 255) & ~255
        buffer = sc.HostBuffer(split + path_bytes + 64)
        buffer.array[:] = 0xEE
        sc._check(sc.lib().sc_merkle_rows_query_dev(tree._h, table, w, idx, k, buffer.ptr, vp(buffer.ptr.value + split)))
        raw = buffer.array.tobytes()
        assert raw[row_bytes:split] == GUARD * (split - row_bytes) and raw[split + path_bytes:] == GUARD * 64
        return raw[:row_bytes], raw[split:split + path_bytes]
    rows, paths = guarded(row_bytes + 64), guarded(path_bytes + 64)
    sc._check(sc.lib().sc_merkle_rows_query_dev(tree._h, table, w, idx, k, rows, paths))
    assert rows.raw[row_bytes:] == GUARD * 64 and paths.raw[path_bytes:] == GUARD * 64
    return rows.raw[:row_bytes], paths.raw[:path_bytes]


def level_of(sc, tree, level):
    out = sc.DeviceVector(4 * (tree.n >> level))
    tree.copy_level(level, out.ptr)
    sc.synchronize()
    return out.to_bytes()


def opened_indices(n):
    if n <= 64:
        return list(range(n))
    rng = random.Random(n)
    return [0, n - 1, n // 2 - 1, n // 2] + [rng.randrange(n) for _ in range(60)]


def check_tree(sc, tree, pointers, columns, levels, pinned=False):
    """the root, every level up to 4096 leaves, and opened rows and paths (all of them up to 64 leaves, 64 otherwise)"""
    n = tree.n
    assert tree.root == levels[-1][0]
    if n <= 4096:
        for l, level in enumerate(levels):
            assert level_of(sc, tree, l) == b"".join(level), "level %d" % l
    indices = opened_indices(n)
    rows, paths = query(sc, tree, pointers, indices, pinned)
    assert rows == b"".join(cases.row_of(columns, i) for i in indices)
    assert paths == b"".join(b"".join(cases.path(levels, i)) for i in indices)
    if n >= 2:                                      # an ordinary sc_merkle_t: the existing opening entry works on it
        assert tree.open_batch(indices[:4]) == [cases.path(levels, i) for i in indices[:4]]


# ---- build and query -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["views", "separate"])
@pytest.mark.parametrize("w", WIDTHS)
def test_widths(sc, w, layout):
    """N = 512 (two workgroups of the fused entry): one column, a partial block, one full block exactly (no empty block behind it), one
    value over, several blocks with a full and a partial last one, and the maximum"""
    columns, levels = cases.reference(w, 512)
    keep, pointers = resident(sc, columns, layout)
    check_tree(sc, build(sc, pointers, 512), pointers, columns, levels, pinned=(layout == "views"))


@pytest.mark.parametrize("w", (3, 9))
@pytest.mark.parametrize("n", SIZES)
def test_sizes(sc, n, w):
    """below the fused entry (1 .. 128: the plain leaf launch), the first fused size (256: the root comes from the subtree launch), with
    and without the tail kernel behind it, 2048 / 4096 (the widest level the tail kernel takes, and one fused climb in front of it),
    2^17 = FUSE_MAX_W (the latency form) and 2^18 (the throughput form, two levels per launch)"""
    columns, levels = cases.reference(w, n)
    layouts = ("views", "separate") if n <= 4096 else (("views",) if w == 3 else ("separate",))
    for layout in layouts:
        keep, pointers = resident(sc, columns, layout)
        check_tree(sc, build(sc, pointers, n), pointers, columns, levels, pinned=(w == 9))


@pytest.mark.parametrize("w,n", [(8, 256), (9, 512), (3, 4)])
def test_columns_of_zero_and_of_p_minus_one(sc, w, n):
    columns, levels = cases.reference(w, n, "extremes")
    keep, pointers = resident(sc, columns, "views")
    check_tree(sc, build(sc, pointers, n), pointers, columns, levels)


@pytest.mark.parametrize("n", (1, 128, 256, 2048, 1 << 17))
def test_async_build_has_the_synchronous_root(sc, n):
    columns, levels = cases.reference(3, n)
    keep, pointers = resident(sc, columns, "separate")
    sc.synchronize()
    later = build(sc, pointers, n, "async")
    assert later.root == build(sc, pointers, n).root == levels[-1][0]


def test_builds_on_two_streams(sc):
    """the header declares the build entries free of the one-stream rule: six asynchronous builds of different columns alternate on two
    caller streams with no host wait in between; every root and every leaf level is the model's"""
    import torch
    streams = [torch.cuda.Stream(device=torch.device("cuda", 0)) for _ in range(2)]
    shapes = [(3, 2048), (9, 512), (17, 4096), (3, 512), (9, 2048), (2, 256)]
    operands = [resident(sc, cases.reference(w, n)[0], "separate") for w, n in shapes]
    sc.synchronize()                                # (the uploads ran on the library's stream)
    trees = [build(sc, pointers, n, "async", vp(streams[k % 2].cuda_stream)) for k, ((w, n), (keep, pointers)) in enumerate(zip(shapes, operands))]
    for (w, n), tree in zip(shapes, trees):
        levels = cases.reference(w, n)[1]
        assert tree.root == levels[-1][0]
    for s in streams:
        s.synchronize()
    for (w, n), tree in zip(shapes, trees):
        assert level_of(sc, tree, 0) == b"".join(cases.reference(w, n)[1][0])


def test_row_tree_class(sc):
    """starkcore.RowTree and Merkle.commit_rows / open_rows on device-sized inputs"""
    from algebra import Field, FieldElement
    from merkle import Merkle
    field = Field.main()
    columns, levels = cases.reference(3, 512)
    ints = [cases.unpack(column) for column in columns]
    lists = [[FieldElement(v, field) for v in column] for column in ints]
    codewords = [sc.DeviceCodeword.from_list(column, field) for column in lists]
    for given in (lists, codewords, [codewords[0], lists[1], codewords[2]]):
        assert Merkle.commit_rows(given) == levels[-1][0]
        row, path = Merkle.open_rows(77, given)
        assert [v.value for v in row] == [column[77] for column in ints] and path == cases.path(levels, 77)
        assert all(v.field is field for v in row) and Merkle.verify_rows(levels[-1][0], 77, path, row) is True
    tree = sc.RowTree.start(codewords)
    assert tree.root == sc.RowTree.build(lists).root == levels[-1][0]
    rows, paths = tree.query([0, 511, 255, 256])
    assert rows == [[column[i] for column in ints] for i in (0, 511, 255, 256)] and paths == [cases.path(levels, i) for i in (0, 511, 255, 256)]
    assert tree.query([]) == ([], [])
    tree.free()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(sc):
    """every refusal returns its code with nothing written: the root buffer, the tree handle, the opened rows and paths keep their
    sentinels"""
    lib = sc.lib()
    columns, levels = cases.reference(3, 512)
    keep, pointers = resident(sc, columns, "separate")
    good = (vp * 3)(*pointers)
    holed = (vp * 3)(pointers[0], None, pointers[2])
    many = (vp * 257)(*([pointers[0]] * 257))
    untouched = 0xDEAD0
    for table, w, n, code in ((good, 0, 512, SC_ERR_BAD_ARG), (many, 257, 512, SC_ERR_BAD_ARG), (holed, 3, 512, SC_ERR_BAD_ARG), (None, 3, 512, SC_ERR_BAD_ARG),
                              (good, 3, 0, SC_ERR_NOT_POW2), (good, 3, 384, SC_ERR_NOT_POW2), (good, 3, 511, SC_ERR_NOT_POW2)):
        root, handle = guarded(64), vp(untouched)
        assert lib.sc_merkle_rows_build_dev(table, w, n, root, ctypes.byref(handle), None) == code
        assert root.raw == GUARD * 64 and handle.value == untouched
        assert lib.sc_merkle_rows_build_async_dev(table, w, n, ctypes.byref(handle), None) == code
        assert handle.value == untouched
    assert lib.sc_merkle_rows_build_async_dev(good, 3, 512, None, None) == SC_ERR_BAD_ARG
    assert lib.sc_merkle_rows_build_dev(good, 3, 512, None, None, None) == SC_ERR_BAD_ARG
    tree = build(sc, pointers, 512)
    rows, paths = guarded(16 * 3 * 2), guarded(64 * 9 * 2)
    for table, w, indices in ((good, 3, (5, 512)), (good, 3, (1 << 63, 0)), (good, 0, (5, 6)), (many, 257, (5, 6)), (holed, 3, (5, 6)), (None, 3, (5, 6))):
        assert lib.sc_merkle_rows_query_dev(tree._h, table, w, (u64 * 2)(*indices), 2, rows, paths) == SC_ERR_BAD_ARG
        assert rows.raw == GUARD * len(rows) and paths.raw == GUARD * len(paths)
    assert lib.sc_merkle_rows_query_dev(None, good, 3, (u64 * 2)(5, 6), 2, rows, paths) == SC_ERR_BAD_ARG
    assert lib.sc_merkle_rows_query_dev(tree._h, good, 3, (u64 * 2)(5, 6), 2, None, paths) == SC_ERR_BAD_ARG
    assert lib.sc_merkle_rows_query_dev(tree._h, good, 3, (u64 * 2)(5, 6), 0, rows, paths) == 0
    assert rows.raw == GUARD * len(rows) and paths.raw == GUARD * len(paths)
    check_tree(sc, tree, pointers, columns, levels)     # and the tree still answers
