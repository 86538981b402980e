"""Row forests without a GPU (csrc/merkle_forest.cuh + csrc/merkle_rows.cuh): tests/emu/row_forest_emu.cpp runs the
SC_HD functions of the kernels -- the segment lookup and address, forest_place, forest_wg_flat, the launch plan, row_leaf_walk -- over
whole small forests, workgroup by workgroup and lane by lane, against the hashlib model of tests/merkle_rows_cases.py: every digest
where forest_path_digest looks for it, every root, no address outside a segment (so the padding lanes of the last workgroup read
nothing), the query kernel's routing; and Merkle.commit_rows_batch below ROWS_DEVICE_MIN, on the host path."""
import ctypes
import os
import struct
import subprocess

import pytest

from conftest import REPO
import merkle_rows_cases as cases
import row_forest_cases as forests

EMU_DIR = os.path.join(REPO, "tests", "emu")
CSRC = os.path.join(REPO, "stark-anatomy_amd", "csrc")
SOURCES = [os.path.join(EMU_DIR, "row_forest_emu.cpp")] + [os.path.join(CSRC, f) for f in ("merkle_rows.cuh", "merkle_forest.cuh", "merkle.cuh", "field.cuh", "transcript.h")]
vp, u64 = ctypes.c_void_p, ctypes.c_uint64
SIZES = (2, 4, 64, 256, 512)
COUNTS = (1, 2, 3, 5, 129)


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(EMU_DIR, "librow_forest_emu.so")
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in SOURCES):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", so, SOURCES[0]])
    lib = ctypes.CDLL(so)
    lib.emu_row_forest_build.restype = ctypes.c_int
    lib.emu_row_forest_build.argtypes = [vp, vp, vp, vp, u64, u64, u64, vp, vp, vp]
    lib.emu_row_forest_query.restype = ctypes.c_int
    lib.emu_row_forest_query.argtypes = [vp, vp, vp, vp, u64, u64, vp, vp, vp, u64, vp, vp]
    return lib


class Table:
    """the segments of a case in host memory, each buffer EXACTLY as long as its matrix: an address past it is outside"""

    def __init__(self, buffers, per_tree, pitch):
        self.keep = [ctypes.create_string_buffer(b, len(b)) for b in buffers]
        s = len(buffers)
        self.bases = (vp * s)(*[ctypes.addressof(b) for b in self.keep])
        self.per_tree = (u64 * s)(*per_tree)
        self.pitch = (u64 * s)(*[pitch] * s)
        self.nbytes = (u64 * s)(*[len(b) for b in buffers])
        self.count = s

    def head(self):
        return self.bases, self.per_tree, self.pitch, self.nbytes, self.count


def build(emu, table, n, count):
    levels = ctypes.create_string_buffer(64 * 2 * n * count)
    roots = ctypes.create_string_buffer(b"\xEE" * (64 * count + 64), 64 * count + 64)
    stats = (u64 * 3)()
    rc = emu.emu_row_forest_build(*table.head(), n, count, levels, roots, stats)
    return rc, levels, roots.raw, list(stats)


def check(emu, layout, n, count, pad):
    buffers, per_tree, pitch, columns, model = forests.forest(layout, n, count, pad)
    table = Table(buffers, per_tree, pitch)
    rc, levels, roots, stats = build(emu, table, n, count)
    assert rc == 0
    w, depth = sum(layout), n.bit_length() - 1
    assert roots[:64 * count] == b"".join(forests.roots(model)) and roots[64 * count:] == b"\xEE" * 64
    # one value per (tree, row, column) and no more: the padding lanes of the last workgroup loaded nothing
    assert stats == [(depth + 7) // 8, sum((count * (n >> l) + 255) // 256 for l in range(0, depth, 8)), count * n * w]
    # every digest below the roots, through the query kernel's own routing: every leaf of every tree at the small sizes
    step = 1 if count * n <= 1024 else max(1, (count * n) // 512) | 1
    positions = [(flat // n, flat % n) for flat in range(0, count * n, step)] + [(count - 1, n - 1)]
    k = len(positions)
    rows = ctypes.create_string_buffer(b"\xEE" * (16 * w * k + 16), 16 * w * k + 16)
    paths = ctypes.create_string_buffer(b"\xEE" * (64 * depth * k + 64), 64 * depth * k + 64)
    trees, indices = (u64 * k)(*[t for t, _ in positions]), (u64 * k)(*[i for _, i in positions])
    assert emu.emu_row_forest_query(*table.head()[:4], table.count, n, levels, trees, indices, k, rows, paths) == 0
    assert rows.raw == b"".join(forests.row(columns, t, i) for t, i in positions) + b"\xEE" * 16
    assert paths.raw == b"".join(forests.path(model, t, i) for t, i in positions) + b"\xEE" * 64
    for t, i in positions[:8]:
        assert cases.verify(model[t][-1][0], i, cases.path(model[t], i), cases.unpack(forests.row(columns, t, i)))


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("n", SIZES)
def test_shapes(emu, n, count):
    """trees that share a workgroup (N = 2: 128 of them, 4: 64, 64: four), one tree per workgroup, two launches (512); the last
    workgroup partly or nearly empty (count 3, 5, 129)"""
    check(emu, (3, 1), n, count, 0)


@pytest.mark.parametrize("pad", (0, 3))
@pytest.mark.parametrize("layout", forests.LAYOUTS, ids=lambda l: "-".join(map(str, l)))
def test_segment_layouts(emu, layout, pad):
    """one segment, the prover's two, segment boundaries inside a block of eight columns and on it, a second block, eight segments"""
    for n, count in ((4, 5), (64, 3), (256, 2)):
        check(emu, layout, n, count, pad)


def test_a_column_read_from_the_wrong_place_changes_a_root(emu):
    """the case builders do what they are for: swapping two trees' columns, or two segments' per_tree, gives other roots"""
    buffers, per_tree, pitch, columns, model = forests.forest((3, 1), 64, 3, 3)
    rc, _, roots, _ = build(emu, Table(buffers, per_tree, pitch), 64, 3)
    assert rc == 0
    swapped = [buffers[0], buffers[1][16 * pitch:32 * pitch] + buffers[1][:16 * pitch] + buffers[1][32 * pitch:]]
    rc, _, other, _ = build(emu, Table(swapped, per_tree, pitch), 64, 3)
    assert rc == 0 and other[:128] != roots[:128] and other[128:192] == roots[128:192]
    rc, _, other, _ = build(emu, Table(buffers, per_tree, pitch - 1), 64, 3)
    assert rc == 0 and other[:64] != roots[:64]


def test_addresses_outside_a_segment_are_caught(emu):
    """the emulator's own guard: a segment one column short, or a tree too many, is a read outside"""
    buffers, per_tree, pitch, _, _ = forests.forest((3, 1), 64, 3, 0)
    short = [buffers[0], buffers[1][:-16]]
    assert build(emu, Table(short, per_tree, pitch), 64, 3)[0] == -2
    assert build(emu, Table(buffers, per_tree, pitch), 64, 4)[0] == -2
    assert build(emu, Table(buffers, [3, 0], pitch), 64, 3)[0] == -3
    assert build(emu, Table(buffers, per_tree, 63), 64, 3)[0] == -3


def test_standalone_walk_under_sanitizers(tmp_path):
    """the emulator with a main of its own, built under ASan + UBSan and run as a program (ROW_FOREST_EMU_CXXFLAGS overrides the
    flags): trees sharing a workgroup with a partly empty last one, two launches, two blocks per row, eight segments, pitch > N"""
    flags = os.environ.get("ROW_FOREST_EMU_CXXFLAGS", "-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer").split()
    program = os.path.join(EMU_DIR, "row_forest_emu_main")
    stale = not os.path.exists(program) or any(os.path.getmtime(s) > os.path.getmtime(program) for s in SOURCES)
    if stale or "ROW_FOREST_EMU_CXXFLAGS" in os.environ:
        subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas", "-DROW_FOREST_EMU_MAIN"] + flags + ["-o", program, SOURCES[0]])
    shapes = [((3, 1), 4, 129, 0), ((16, 1), 64, 5, 3), ((7, 3), 512, 2, 0), ((1,) * 8, 256, 3, 3), ((1,), 2, 1, 0)]
    call = b""
    for layout, n, count, pad in shapes:
        buffers, per_tree, pitch, _, _ = forests.forest(layout, n, count, pad)
        call += struct.pack("<4Q", len(layout), n, count, pitch) + struct.pack("<%dQ" % len(layout), *per_tree) + b"".join(buffers)
    path = tmp_path / "forests.bin"
    path.write_bytes(call)
    done = subprocess.run([program, str(path)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert done.returncode == 0, done.stderr[-2000:]
    lines = done.stdout.split("\n")
    assert len(lines) == len(shapes) + 1 and lines[-1] == ""
    for (layout, n, count, pad), line in zip(shapes, lines):
        model = forests.forest(layout, n, count, pad)[4]
        assert bytes.fromhex(line) == b"".join(forests.roots(model)) + forests.path(model, count - 1, n - 1)


# ---- Merkle.commit_rows_batch on the host path -----------------------------------------------------------------------------------------
def fe(values):
    from algebra import Field, FieldElement
    field = Field.main()
    return [FieldElement(v, field) for v in values]


@pytest.mark.parametrize("w,n,count", [(1, 1, 3), (3, 2, 2), (4, 8, 5), (9, 16, 3), (17, 4, 1)])
def test_commit_rows_batch_below_the_device_threshold(w, n, count):
    from merkle import Merkle
    assert count * n < Merkle.ROWS_DEVICE_MIN
    ints = [cases.matrix(w, n, seed=1000 * t + 7) for t in range(count)]
    members = [[fe(column) for column in member] for member in ints]
    roots = Merkle.commit_rows_batch(members)
    assert roots == [cases.levels(member)[-1][0] for member in ints] == [Merkle.commit_rows(member) for member in members]


def test_commit_rows_batch_of_unequal_members_and_of_none():
    from merkle import Merkle
    ints = [cases.matrix(3, 8), cases.matrix(2, 8), cases.matrix(3, 4)]
    members = [[fe(column) for column in member] for member in ints]
    assert Merkle.commit_rows_batch(members) == [cases.levels(member)[-1][0] for member in ints]
    assert Merkle.commit_rows_batch([]) == []
    with pytest.raises(AssertionError):
        Merkle.commit_rows_batch([members[0], [members[0][0], members[0][1][:4]]])
