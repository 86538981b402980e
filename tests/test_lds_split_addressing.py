"""The LDS addressing of the eight-element batch kernels (csrc/ntt_tile.cuh, Round::gather_lds_split / scatter_lds_split: one lane
address per exchange side, the rest compile-time) against the per-element form of the generic and emulated paths, on the CPU:
tests/emu/lds_split_check.cpp walks every shape, round, thread and element."""
import os
import re
import subprocess

from conftest import REPO


def test_split_addresses_equal_the_per_element_ones(tmp_path):
    exe = str(tmp_path / "lds_split_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(REPO, "tests", "emu", "lds_split_check.cpp")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    lines = run.stdout.splitlines()
    assert run.returncode == 0, run.stdout
    # three shapes; (10,2) has four rounds, the others three; the first round of each in both splits of the thread index
    assert len(lines) == (4 + 1) + (3 + 1) + (3 + 1)
    for line in lines:
        m = re.match(r"fixed8<(\d+),(\d+)> round (\d+) \(S (\d+), sh (\d+)\) rfast ([01]): (\d+) mismatches, (\d+) lane bases, max offset (\d+) bytes$", line)
        assert m, line
        logr, logc, _, _, sh, _, bad, bases, off = map(int, m.groups())
        assert bad == 0 and off < 65536
        # the swizzle's compile-time bits: none when the round's row bits lie above the column bits
        assert 1 <= bases <= (1 << logc)
        if sh >= logc and not int(m.group(6)):
            assert bases == 1, line
    # the gather of the last round (sh = 0) of the benchmark's shape needs four lane bases, not eight addresses
    assert any(l.startswith("fixed8<10,2> round 3 (S 3, sh 0) rfast 0: 0 mismatches, 4 lane bases") for l in lines)
