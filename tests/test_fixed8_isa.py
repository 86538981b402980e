"""The eight-element batch kernels (ntt_pass_kernel_fixed8) as built: their global accesses on the plain path are addressed as SGPR
base + 32-bit VGPR offset, nothing goes through scratch, and the hazard padding and the index arithmetic do not grow past what the
kernels reach now (tools/fixed8_isa.py; static counts over every variant path).  CPU only: reads the built library's gfx950 code object."""
import importlib.util
import os

import pytest

from conftest import REPO

LIB = os.path.join(REPO, "stark-anatomy_amd", "libstarkcore.so")
# per kernel <LR, LC>: ceilings of the static counts of the current build
CEIL = {"10,2": {"s_nop": 3413, "b_other": 376, "scratch": 0},
        "9,3": {"s_nop": 3833, "b_other": 401, "scratch": 0},
        "8,4": {"s_nop": 3509, "b_other": 408, "scratch": 0}}


def _tool():
    spec = importlib.util.spec_from_file_location("fixed8_isa", os.path.join(REPO, "tools", "fixed8_isa.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def mix():
    if not os.path.exists(LIB):
        pytest.skip("libstarkcore.so not built")
    t = _tool()
    if not all(t.tool(x) for x in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump")):
        pytest.skip("LLVM binutils not found")
    return {"%d,%d" % k: t.counts(v) for k, v in t.kernels(t.disassemble(LIB)).items()}


def test_every_fixed8_shape_is_built(mix):
    assert set(mix) == set(CEIL)


@pytest.mark.parametrize("shape", sorted(CEIL))
def test_fixed8_addressing_and_ceilings(mix, shape):
    c = mix[shape]
    assert c["st_vaddr"] == 0, c                    # every store: s[base] + v_offset
    assert c["g_saddr"] >= 24, c                    # data loads, direct twiddle loads and stores of the plain path (8 each)
    for k, ceil in CEIL[shape].items():
        assert c[k] <= ceil, (shape, k, c[k], ceil)
