"""Row commitments without a GPU (csrc/merkle_rows.cuh, merkle.py): the specification against hashlib, the block walk
the kernels run -- compiled for the host by tests/emu/merkle_rows_emu.cpp over transcript.h's compression -- and the library's
host-only sc_merkle_row_leaf at every width of tests/merkle_rows_cases.py, the walk once more as a stand-alone program under ASan +
UBSan (MERKLE_ROWS_EMU_CXXFLAGS overrides the flags), and the host bodies of Merkle.commit_rows / open_rows / verify_rows on small
trees.  (FastStark(row_commitments=True) on the host-list data flow needs the GPU behind its fast_* calls: tests/test_gpu_merkle_rows.py.)"""
import ctypes
import os
import struct
import subprocess
from hashlib import blake2b

import pytest

from conftest import REPO
import merkle_rows_cases as cases
from merkle_rows_cases import P

EMU_DIR = os.path.join(REPO, "tests", "emu")
CSRC = os.path.join(REPO, "stark-anatomy_amd", "csrc")
SOURCES = [os.path.join(EMU_DIR, "merkle_rows_emu.cpp")] + [os.path.join(CSRC, f) for f in ("merkle_rows.cuh", "merkle.cuh", "field.cuh", "transcript.h")]
SC_ERR_BAD_ARG = -6              # include/starkcore.h
ROWS = 8                         # rows per matrix: the five special values in every column, then random ones


def stale(target):
    return not os.path.exists(target) or any(os.path.getmtime(s) > os.path.getmtime(target) for s in SOURCES)


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(EMU_DIR, "libmerkle_rows_emu.so")
    if stale(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", so, SOURCES[0]])
    lib = ctypes.CDLL(so)
    lib.emu_row_leaves.restype = ctypes.c_int
    lib.emu_row_leaves.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]
    return lib


def fe(values):
    from algebra import Field, FieldElement
    field = Field.main()
    return [FieldElement(v, field) for v in values]


def test_row_leaf_is_the_personalised_hash():
    from merkle import Merkle
    for w in cases.CPU_WIDTHS:
        for row in zip(*cases.matrix(w, ROWS)):
            raw = b"".join(v.to_bytes(16, "little") for v in row)
            assert Merkle.row_leaf(fe(row)) == blake2b(raw, person=b"sc-merkle-row").digest() == cases.leaf(row)


def test_row_leaf_is_neither_the_plain_hash_nor_a_node():
    """a row of 8 values is 128 bytes, the length of a node's message: the personalisation keeps the two apart"""
    from merkle import Merkle
    row = list(zip(*cases.matrix(8, ROWS)))[5]
    raw = b"".join(v.to_bytes(16, "little") for v in row)
    left, right = raw[:64], raw[64:]
    assert len(raw) == 128
    assert Merkle.row_leaf(fe(row)) != blake2b(raw).digest()
    assert Merkle.row_leaf(fe(row)) != Merkle.H(left + right).digest()
    assert Merkle.commit_rows([fe([v]) for v in row]) != Merkle.commit_([left, right])


@pytest.mark.parametrize("w", cases.CPU_WIDTHS)
def test_block_walk_on_the_host(emu, w):
    """the kernels' walk (blocks, message words, counter, final flag, initial state), lane by lane over a table of column pointers"""
    columns = cases.matrix(w, ROWS)
    buffers = [ctypes.create_string_buffer(cases.pack(column)) for column in columns]
    table = (ctypes.c_void_p * w)(*[ctypes.addressof(b) for b in buffers])
    out = ctypes.create_string_buffer(64 * ROWS + 64)
    out.raw = b"\xEE" * len(out)
    assert emu.emu_row_leaves(table, w, ROWS, out) == 0
    assert [out.raw[64 * i:64 * i + 64] for i in range(ROWS)] == [cases.leaf(row) for row in zip(*columns)]
    assert out.raw[64 * ROWS:64 * ROWS + 64] == b"\xEE" * 64


def test_block_walk_refuses_bad_widths(emu):
    out = ctypes.create_string_buffer(b"\xEE" * 64)
    one = ctypes.create_string_buffer(16)
    for w in (0, 257):
        table = (ctypes.c_void_p * max(w, 1))(*[ctypes.addressof(one)] * max(w, 1))
        assert emu.emu_row_leaves(table, w, 1, out) == 1 and out.raw[:64] == b"\xEE" * 64


@pytest.mark.parametrize("w", cases.CPU_WIDTHS)
def test_library_row_leaf(w):
    """sc_merkle_row_leaf: the same walk inside libstarkcore.so, host only"""
    import starkcore as sc
    lib = sc.lib()
    for row in zip(*cases.matrix(w, ROWS)):
        out = ctypes.create_string_buffer(b"\xEE" * 128)
        assert lib.sc_merkle_row_leaf(cases.pack(row), w, out) == 0
        assert out.raw[:64] == cases.leaf(row) and out.raw[64:128] == b"\xEE" * 64


def test_library_row_leaf_refusals():
    import starkcore as sc
    lib = sc.lib()
    out = ctypes.create_string_buffer(b"\xEE" * 64)
    row = bytes(16 * 257)
    for args in ((row, 0, out), (row, 257, out), (None, 3, out), (row, 3, None)):
        assert lib.sc_merkle_row_leaf(*args) == SC_ERR_BAD_ARG
    assert out.raw[:64] == b"\xEE" * 64


def test_standalone_walk_under_sanitizers(tmp_path):
    """the walk with a main of its own, built under ASan + UBSan and run as a program: one, eight, nine and 256 columns"""
    flags = os.environ.get("MERKLE_ROWS_EMU_CXXFLAGS", "-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer").split()
    program = os.path.join(EMU_DIR, "merkle_rows_emu_main")
    if stale(program) or "MERKLE_ROWS_EMU_CXXFLAGS" in os.environ:
        subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas", "-DMERKLE_ROWS_EMU_MAIN"] + flags + ["-o", program, SOURCES[0]])
    widths = (1, 8, 9, 24, 25, 256)
    call = b"".join(struct.pack("<QQ", w, ROWS) + b"".join(cases.pack(column) for column in cases.matrix(w, ROWS)) for w in widths)
    path = tmp_path / "matrices.bin"
    path.write_bytes(call)
    done = subprocess.run([program, str(path)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert done.returncode == 0, done.stderr[-2000:]
    lines = done.stdout.split("\n")
    for w, line in zip(widths, lines):
        assert bytes.fromhex(line) == b"".join(cases.leaf(row) for row in zip(*cases.matrix(w, ROWS)))
    assert len(lines) == len(widths) + 1 and lines[-1] == ""


@pytest.mark.parametrize("w", (1, 3, 9))
@pytest.mark.parametrize("n", (1, 2, 4, 8, 16))
def test_host_trees(w, n):
    """Merkle.commit_rows / open_rows / verify_rows, host bodies, against the model: every index opens and verifies, and a flipped value
    in any column, a swapped pair of columns, a wrong index, a shortened path and a path with an extra digest are rejected"""
    from merkle import Merkle
    ints = cases.matrix(w, n)
    columns = [fe(column) for column in ints]
    model = cases.levels(ints)
    root = Merkle.commit_rows(columns)
    assert root == model[-1][0]
    one = columns[0][0].field.one()
    for index in range(n):
        row, path = Merkle.open_rows(index, columns)
        assert [v.value for v in row] == [column[index] for column in ints] and path == cases.path(model, index)
        assert Merkle.verify_rows(root, index, path, row) is True
        assert cases.verify(root, index, path, [v.value for v in row])
        for c in range(w):
            flipped = row[:c] + [row[c] + one] + row[c + 1:]
            assert Merkle.verify_rows(root, index, path, flipped) is False
        for c in range(w - 1):
            swapped = row[:c] + [row[c + 1], row[c]] + row[c + 2:]
            assert swapped != row and Merkle.verify_rows(root, index, path, swapped) is False
        if n > 1:
            assert Merkle.verify_rows(root, (index + 1) % n, path, row) is False
            assert Merkle.verify_rows(root, index >> 1, path[:-1], row) is False
        extended = path + [bytes(64)]
        assert Merkle.verify_rows(root, index, extended, row) is False


def test_host_trees_refuse_bad_shapes():
    from merkle import Merkle
    columns = [fe(column) for column in cases.matrix(2, 4)]
    for bad in ([], [columns[0], columns[1][:2]], [c[:3] for c in columns]):
        with pytest.raises(AssertionError):
            Merkle.commit_rows(bad)
    for index in (-1, 4):
        with pytest.raises(AssertionError):
            Merkle.open_rows(index, columns)
