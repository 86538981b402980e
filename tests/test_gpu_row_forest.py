"""Row forests on the GPU (csrc/merkle_forest.cuh's forest_climb_kernel with the row leaf stage of csrc/merkle_rows.cuh,
row_forest_query_kernel, csrc/merkle_rows.hip): sc_merkle_row_forest_build_dev / _query_dev against the hashlib model
of tests/merkle_rows_cases.py over the layouts of tests/row_forest_cases.py -- every shape at which the kernel takes another path
(trees sharing a workgroup, a last workgroup partly empty, one / two / three launches), every width class of the block walk, every
segment layout, both forms of the narrow levels, answers into sentinel-guarded pinned and ordinary buffers, the refusals, two streams,
and the Python wrappers (starkcore.RowForest, Merkle.commit_rows_batch).  The batched provers: tests/test_gpu_row_forest_proofs.py."""
import ctypes
import random

import pytest

import merkle_rows_cases as cases
import row_forest_cases as forests

pytestmark = pytest.mark.gpu
vp, u64 = ctypes.c_void_p, ctypes.c_uint64
GUARD = b"\xEE"
SC_ERR_NOT_POW2, SC_ERR_BAD_ARG, SC_ERR_UNSUPPORTED = -2, -6, -7          # include/starkcore.h
FOREST_MAX_LEAVES = 1 << 24


@pytest.fixture(scope="module")
def sc():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible: the HIP path is mandatory for these tests"
    starkcore.init()
    return starkcore


# ---- helpers ---------------------------------------------------------------------------------------------------------------------------
def guarded(nbytes):
    return ctypes.create_string_buffer(GUARD * nbytes, nbytes)


class Resident:
    """a case's segments in HBM, every segment an allocation of its own, and the table that describes them"""

    def __init__(self, sc, case):
        buffers, per_tree, pitch, self.columns, self.levels = case
        self.vectors = [sc.DeviceVector.from_bytes(b) for b in buffers]
        self.table = (sc.RowSegment * len(buffers))()
        for entry, vector, per in zip(self.table, self.vectors, per_tree):
            entry.base, entry.per_tree, entry.pitch = vector.ptr, per, pitch
        self.w = sum(per_tree)


def build(sc, resident, n, count, stream=None):
    handle = vp()
    sc._check(sc.lib().sc_merkle_row_forest_build_dev(resident.table, len(resident.table), n, count, ctypes.byref(handle), stream))
    return handle


def roots_of(sc, handle, count):
    out = guarded(64 * count + 64)
    sc._check(sc.lib().sc_merkle_forest_roots(handle, out))
    assert out.raw[64 * count:] == GUARD * 64
    return out.raw[:64 * count]


def query(sc, handle, resident, n, positions, pinned=False):
    """sc_merkle_row_forest_query_dev into guarded buffers -> (rows bytes, paths bytes); pinned: one buffer of sc_host_alloc, which the
    kernel writes itself"""
    w, k, depth = resident.w, len(positions), n.bit_length() - 1
    row_bytes, path_bytes = 16 * k * w, 64 * depth * k
    trees, idx = (u64 * max(k, 1))(*[t for t, _ in positions]), (u64 * max(k, 1))(*[i for _, i in positions])
    lib, table = sc.lib(), resident.table
    if pinned:
        split = (row_bytes + 64 + 255) & ~255
        buffer = sc.HostBuffer(split + path_bytes + 64)
        buffer.array[:] = 0xEE
        sc._check(lib.sc_merkle_row_forest_query_dev(handle, table, len(table), trees, idx, k, buffer.ptr, vp(buffer.ptr.value + split)))
        raw = buffer.array.tobytes()
        assert raw[row_bytes:split] == GUARD * (split - row_bytes) and raw[split + path_bytes:] == GUARD * 64
        return raw[:row_bytes], raw[split:split + path_bytes]
    rows, paths = guarded(row_bytes + 64), guarded(path_bytes + 64)
    sc._check(lib.sc_merkle_row_forest_query_dev(handle, table, len(table), trees, idx, k, rows, paths))
    assert rows.raw[row_bytes:] == GUARD * 64 and paths.raw[path_bytes:] == GUARD * 64
    return rows.raw[:row_bytes], paths.raw[:path_bytes]


def all_leaves(n, count):
    return [(t, i) for t in range(count) for i in range(n)]


def seeded_positions(n, count, per_tree=64):
    rng = random.Random(n + count)
    return [(t, i) for t in range(count) for i in [0, n - 1] + [rng.randrange(n) for _ in range(per_tree)]]


def check_answers(resident, positions, rows, paths):
    assert rows == b"".join(forests.row(resident.columns, t, i) for t, i in positions)
    assert paths == b"".join(forests.path(resident.levels, t, i) for t, i in positions)


def check_forest(sc, case, n, count, positions=None, pinned=False):
    """the roots, and rows and paths at `positions` (default: every leaf of every tree, which touches every node below the roots)"""
    lib = sc.lib()
    resident = Resident(sc, case)
    before = sc.forest_stats()
    handle = build(sc, resident, n, count)
    try:
        assert sc.forest_stats() == (before[0] + 1, before[1] + count)
        assert lib.sc_merkle_forest_trees(handle) == count and lib.sc_merkle_forest_leaves(handle) == n
        assert roots_of(sc, handle, count) == b"".join(forests.roots(resident.levels))
        positions = all_leaves(n, count) if positions is None else positions
        check_answers(resident, positions, *query(sc, handle, resident, n, positions, pinned))
    finally:
        sc._check(lib.sc_merkle_forest_free(handle))


# ---- roots and every path --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,count", [(2, 3), (2, 257), (4, 129), (64, 5), (256, 1), (256, 3), (512, 3), (4096, 3)])
def test_shapes(sc, n, count):
    """N = 2 and 4: 128 and 64 trees per workgroup (count 257 crosses a workgroup at one leaf pair); N = 64, count 5: the last
    workgroup a quarter full; N = 256: one tree per workgroup, one launch; 512: the first second launch (levels 8 - 9); 2^12 with three
    trees: the signature's shape.  Every leaf of every tree is opened."""
    check_forest(sc, forests.forest((2, 1), n, count), n, count, pinned=(count % 2 == 1))


def test_three_launches(sc):
    """N = 2^17: levels 0 - 8, 8 - 16, 16 - 17; 64 seeded positions per tree plus the first and the last row"""
    n, count = 1 << 17, 2
    check_forest(sc, forests.forest((2, 1), n, count), n, count, seeded_positions(n, count), pinned=True)


# ---- widths and segments ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", (1, 7, 8, 9, 16, 17, 256))
def test_widths(sc, w):
    """one column, a partial block, a full block that is the final one, one value over, two full blocks, a third block, the maximum"""
    n, count = 256, (2 if w == 256 else 3)
    check_forest(sc, forests.forest((w,), n, count), n, count, seeded_positions(n, count, 16), pinned=(w % 2 == 0))


@pytest.mark.parametrize("pad", (0, 3))
@pytest.mark.parametrize("layout", forests.LAYOUTS, ids=lambda l: "-".join(map(str, l)))
def test_segment_layouts(sc, layout, pad):
    """segment boundaries inside a block of eight columns, on it and behind it, eight segments; pitch = N and pitch > N (the filler
    between two columns is never read); every segment an allocation of its own"""
    n, count = 256, 3
    check_forest(sc, forests.forest(layout, n, count, pad), n, count, seeded_positions(n, count, 16))


@pytest.mark.parametrize("layout,n,count", [((8,), 256, 3), ((8, 1), 512, 2), ((2, 1), 4, 5)])
def test_columns_of_zero_and_of_p_minus_one(sc, layout, n, count):
    check_forest(sc, forests.forest(layout, n, count, 0, "extremes"), n, count, seeded_positions(n, count, 8))


# ---- four lanes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", (3, 300))
def test_four_lane_levels_change_nothing(sc, count):
    """forest_four_lane_wgs at 0 (never), the default and 2^20 (always, where a launch climbs two levels or more): the same roots and
    the same answers -- 48 resp. 4800 workgroups in the first launch, 1 resp. 19 in the second.  Trees 0, 1 and the last against the
    model, every tree against the other settings."""
    n = 1 << 12
    resident = Resident(sc, forests.forest((2, 1), n, count, 0, "bytes"))
    modelled = sorted({0, 1, count - 1})
    positions = [(t, i) for t in modelled for i in (0, 1, n // 2, n - 1, 1234)]
    seen = []
    try:
        for setting in (0, 256, 1 << 20):
            sc.set_tuning("forest_four_lane_wgs", setting)
            handle = build(sc, resident, n, count)
            roots = roots_of(sc, handle, count)
            answers = query(sc, handle, resident, n, positions, pinned=True)
            sc._check(sc.lib().sc_merkle_forest_free(handle))
            seen.append((roots, answers))
    finally:
        sc.set_tuning("forest_four_lane_wgs", 256)
    assert seen[0] == seen[1] == seen[2]
    roots, (rows, paths) = seen[0]
    assert [roots[64 * t:64 * t + 64] for t in modelled] == [resident.levels[t][-1][0] for t in modelled]
    check_answers(resident, positions, rows, paths)


# ---- query -----------------------------------------------------------------------------------------------------------------------------
def test_query_forms(sc):
    """duplicate, unsorted and single positions, none at all, pinned and ordinary outputs"""
    n, count = 512, 3
    resident = Resident(sc, forests.forest((3, 1), n, count, 3))
    handle = build(sc, resident, n, count)
    for positions in ([(2, 511), (0, 0), (1, 77), (2, 511), (0, 1), (0, 0)], [(1, 300)], []):
        for pinned in (False, True):
            check_answers(resident, positions, *query(sc, handle, resident, n, positions, pinned))
    # the [k][w] rows are the columns
    rows, _ = query(sc, handle, resident, n, [(t, 5) for t in range(count)])
    assert cases.unpack(rows) == [cases.unpack(column)[5] for t in range(count) for column in resident.columns[t]]
    sc._check(sc.lib().sc_merkle_forest_free(handle))


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(sc):
    """every refusal returns its code, leaves sc_merkle_forest_stats as it was and writes nothing: the handle and the guarded outputs
    keep their values"""
    lib = sc.lib()
    n, count = 512, 3
    resident = Resident(sc, forests.forest((3, 1), n, count))
    base = [v.ptr for v in resident.vectors]

    def table(*segments):
        out = (sc.RowSegment * max(len(segments), 1))()
        for entry, (pointer, per, pitch) in zip(out, segments):
            entry.base, entry.per_tree, entry.pitch = pointer, per, pitch
        return out

    good = table((base[0], 3, n), (base[1], 1, n))
    nine = table(*[(base[1], 1, n)] * 9)
    wide = table((base[0], 200, n), (base[0], 57, n))
    stats, untouched = sc.forest_stats(), 0xDEAD0
    refused = [(None, 2, n, count, SC_ERR_BAD_ARG), (good, 0, n, count, SC_ERR_BAD_ARG), (nine, 9, n, count, SC_ERR_BAD_ARG),
               (table((base[0], 3, n), (None, 1, n)), 2, n, count, SC_ERR_BAD_ARG), (table((base[0], 3, n), (base[1], 0, n)), 2, n, count, SC_ERR_BAD_ARG),
               (wide, 2, n, count, SC_ERR_BAD_ARG), (table((base[0], 3, n), (base[1], 1, n - 1)), 2, n, count, SC_ERR_BAD_ARG),
               (good, 2, 1, count, SC_ERR_BAD_ARG), (good, 2, 0, count, SC_ERR_BAD_ARG), (good, 2, n, 0, SC_ERR_BAD_ARG),
               (good, 2, 384, count, SC_ERR_NOT_POW2), (good, 2, 511, count, SC_ERR_NOT_POW2),
               (table((base[0], 3, 1 << 20), (base[1], 1, 1 << 20)), 2, 1 << 20, 17, SC_ERR_UNSUPPORTED), (good, 2, n, FOREST_MAX_LEAVES // n + 1, SC_ERR_UNSUPPORTED)]
    for segments, n_segs, leaves, trees, code in refused:
        handle = vp(untouched)
        assert lib.sc_merkle_row_forest_build_dev(segments, n_segs, leaves, trees, ctypes.byref(handle), None) == code, (n_segs, leaves, trees)
        assert handle.value == untouched and sc.forest_stats() == stats
    assert lib.sc_merkle_row_forest_build_dev(good, 2, n, count, None, None) == SC_ERR_BAD_ARG and sc.forest_stats() == stats
    handle = build(sc, resident, n, count)
    stats = sc.forest_stats()
    rows, paths = guarded(16 * 4 * 2), guarded(64 * 9 * 2)
    two = lambda a, b: (u64 * 2)(a, b)
    for segments, n_segs, trees, indices in ((good, 2, two(0, count), two(5, 6)), (good, 2, two(0, 1), two(5, n)), (good, 2, two(1 << 63, 0), two(5, 6)),
                                             (good, 2, two(0, 1), two(1 << 63, 6)), (None, 2, two(0, 1), two(5, 6)), (good, 0, two(0, 1), two(5, 6)),
                                             (nine, 9, two(0, 1), two(5, 6)), (wide, 2, two(0, 1), two(5, 6)), (good, 2, None, two(5, 6)), (good, 2, two(0, 1), None),
                                             (table((base[0], 3, n), (base[1], 1, n - 1)), 2, two(0, 1), two(5, 6))):
        assert lib.sc_merkle_row_forest_query_dev(handle, segments, n_segs, trees, indices, 2, rows, paths) == SC_ERR_BAD_ARG
        assert rows.raw == GUARD * len(rows) and paths.raw == GUARD * len(paths)
    assert lib.sc_merkle_row_forest_query_dev(None, good, 2, two(0, 1), two(5, 6), 2, rows, paths) == SC_ERR_BAD_ARG
    assert lib.sc_merkle_row_forest_query_dev(handle, good, 2, two(0, 1), two(5, 6), 2, None, paths) == SC_ERR_BAD_ARG
    assert lib.sc_merkle_row_forest_query_dev(handle, good, 2, two(0, 1), two(5, 6), 2, rows, None) == SC_ERR_BAD_ARG
    assert lib.sc_merkle_row_forest_query_dev(handle, good, 2, two(0, 1), two(5, 6), 0, rows, paths) == 0
    assert lib.sc_merkle_row_forest_query_dev(handle, good, 2, None, None, 0, None, None) == 0
    assert rows.raw == GUARD * len(rows) and paths.raw == GUARD * len(paths) and sc.forest_stats() == stats
    positions = seeded_positions(n, count, 8)                                 # and the forest still answers
    check_answers(resident, positions, *query(sc, handle, resident, n, positions))
    sc._check(lib.sc_merkle_forest_free(handle))


# ---- streams ---------------------------------------------------------------------------------------------------------------------------
def test_builds_on_two_streams(sc):
    """the header declares the build free of the one-stream rule: six builds of different forests alternate on two caller streams with
    no host wait in between; roots and answers are the single-stream builds', byte for byte (and the model's)"""
    import torch
    streams = [torch.cuda.Stream(device=torch.device("cuda", 0)) for _ in range(2)]
    shapes = [((3, 1), 2048, 3), ((8, 1), 512, 5), ((16, 1), 4096, 2), ((1,), 64, 9), ((7, 3), 256, 4), ((2, 1), 4096, 3)]
    operands = [Resident(sc, forests.forest(layout, n, count)) for layout, n, count in shapes]
    sc.synchronize()                                # (the uploads ran on the library's stream)
    handles = [build(sc, resident, n, count, vp(streams[k % 2].cuda_stream)) for k, ((_, n, count), resident) in enumerate(zip(shapes, operands))]
    for (_, n, count), resident, handle in zip(shapes, operands, handles):
        positions = seeded_positions(n, count, 8)
        in_flight = (roots_of(sc, handle, count), query(sc, handle, resident, n, positions))
        alone = build(sc, resident, n, count)
        assert in_flight == (roots_of(sc, alone, count), query(sc, alone, resident, n, positions))
        assert in_flight[0] == b"".join(forests.roots(resident.levels))
        check_answers(resident, positions, *in_flight[1])
        sc._check(sc.lib().sc_merkle_forest_free(alone))
    for s in streams:
        s.synchronize()
    for handle in handles:
        sc._check(sc.lib().sc_merkle_forest_free(handle))


# ---- Python wrappers -------------------------------------------------------------------------------------------------------------------
def test_row_forest_class(sc):
    n, count = 512, 3
    buffers, per_tree, pitch, columns, levels = forests.forest((3, 1), n, count, 3)
    vectors = [sc.DeviceVector.from_bytes(b) for b in buffers]
    before = sc.forest_stats()
    forest = sc.RowForest.build([(vectors[0], 3, pitch), (vectors[1], 1, pitch)], n, count)
    assert sc.forest_stats() == (before[0] + 1, before[1] + count)
    assert (forest.width, forest.depth, forest.count, forest.n) == (4, 9, count, n)
    assert forest.roots == forests.roots(levels)
    positions = [(2, 511), (0, 0), (1, 77), (2, 511)]
    rows, paths = forest.query(positions)
    assert rows == [cases.unpack(forests.row(columns, t, i)) for t, i in positions]
    assert paths == [cases.path(levels[t], i) for t, i in positions]
    values, raw_paths = forest.query_raw(positions)
    assert values.tobytes() == b"".join(forests.row(columns, t, i) for t, i in positions) and raw_paths.shape == (4, 64 * 9)
    assert raw_paths.tobytes() == b"".join(forests.path(levels, t, i) for t, i in positions)
    assert forest.query([]) == ([], [])
    with pytest.raises(AssertionError):
        forest.query([(3, 0)])
    # a CodewordMatrix as a segment, the default pitch
    plain = forests.forest((2,), 256, 2)
    matrix = sc.CodewordMatrix(4, 256, sc.DeviceVector.from_bytes(plain[0][0]))
    assert sc.RowForest.build([(matrix, 2)], 256, 2).roots == forests.roots(plain[4])
    forest.free()
    forest.free()


def test_commit_rows_batch_on_the_device(sc, monkeypatch):
    """equal-shape members from ROWS_DEVICE_MIN rows in all: one forest (host lists in one upload, device members copied, mixed); unequal
    members and a batch below the threshold: member by member, no forest"""
    from algebra import Field, FieldElement
    from merkle import Merkle
    field = Field.main()

    def members_of(w, n, count):
        _, _, _, columns, levels = forests.forest((w,), n, count)
        lists = [[[FieldElement(v, field) for v in cases.unpack(column)] for column in columns[t]] for t in range(count)]
        return lists, forests.roots(levels)

    for w, n, count in ((3, 128, 2), (3, 256, 1), (9, 512, 3)):
        lists, roots = members_of(w, n, count)
        assert count * n >= Merkle.ROWS_DEVICE_MIN
        before = sc.forest_stats()
        assert Merkle.commit_rows_batch(lists) == roots
        assert sc.forest_stats() == (before[0] + 1, before[1] + count)
        device = [[sc.DeviceCodeword.from_list(column, field) for column in member] for member in lists]
        mixed = [device[0]] + [[device[t][0]] + lists[t][1:] for t in range(1, count)]
        assert Merkle.commit_rows_batch(device) == roots and Merkle.commit_rows_batch(mixed) == roots
        assert sc.forest_stats() == (before[0] + 3, before[1] + 3 * count)
        assert roots == [Merkle.commit_rows(member) for member in lists]
    first, roots_first = members_of(3, 256, 2)
    second, roots_second = members_of(2, 256, 1)
    third, roots_third = members_of(3, 64, 3)
    before = sc.forest_stats()
    assert Merkle.commit_rows_batch(first + second) == roots_first + roots_second
    assert Merkle.commit_rows_batch(first[:1] + third[:1]) == roots_first[:1] + roots_third[:1]
    assert Merkle.commit_rows_batch(third) == roots_third                     # 192 rows in all: below the threshold
    assert sc.forest_stats() == before
    # a batch above the library's forest limit is split
    monkeypatch.setattr(sc, "FOREST_MAX_LEAVES", 256)
    assert Merkle.commit_rows_batch(first) == roots_first
    assert sc.forest_stats() == (before[0] + 2, before[1] + 2)
