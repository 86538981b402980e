#!/usr/bin/env python3
"""Instruction mix of the eight-element batch kernels (ntt_pass_kernel_fixed8<LR, LC>) in a built libstarkcore.so.

Extracts the gfx950 code object of core.hip from the library's .hip_fatbin section, disassembles it with llvm-objdump and counts,
per kernel, the instruction classes that set the kernel's time:

  field    4-cycle ("class B") VALU of the field arithmetic: v_mad_u64_u32, the carry / borrow adds, v_cndmask_b32_e64
  b_other  other 4-cycle VALU: 64-bit and three-operand forms (v_lshl_add_u64, v_mov_b64, v_mul_lo_u32, v_add3_u32, ...) --
           nearly all of it index and address arithmetic
  a        2-cycle VALU (class A)
  s_nop    hazard padding
  scratch  scratch_* instructions (a spill)
  g_vaddr  global loads / stores addressed by a 64-bit VGPR pair (an address built per access on the VALU)
  g_saddr  global loads / stores addressed as SGPR base + 32-bit VGPR offset
  st_vaddr the stores among g_vaddr

Static counts over the whole kernel body (every variant path: coset scaling, zero padding, pruning, twiddle-on-load, ...); the
executed stream of a launch is measured with rocprofv3 --pmc (SQ_INSTS_VALU), see DESIGN.md 3.1.

  python3 tools/fixed8_isa.py [--lib stark-anatomy_amd/libstarkcore.so] [--json]
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_RE = re.compile(r"^[0-9a-f]+ <(_Z\d+ntt_pass_kernel_fixed8ILi(\d+)ELi(\d+)E\w*)>:")

FIELD = {"v_mad_u64_u32", "v_addc_co_u32_e64", "v_subb_co_u32_e64", "v_add_co_u32_e64", "v_sub_co_u32_e64", "v_cndmask_b32_e64"}
# 4-cycle VALU forms outside the field arithmetic (VOP3 64-bit / three-operand / 32-bit multiplies)
B_OTHER_PREFIX = ("v_lshl_add_u64", "v_mov_b64", "v_lshl_add_u32", "v_mul_lo_u32", "v_mul_hi_u32", "v_add3_u32", "v_lshlrev_b64",
                  "v_lshrrev_b64", "v_ashrrev_i64", "v_cmp_", "v_mad_u32", "v_bfe_u32", "v_bitop3", "v_lshl_or_b32", "v_and_or_b32",
                  "v_or3_b32", "v_alignbit", "v_perm_b32", "v_add_u64", "v_sub_u64", "v_mad_i64", "v_add_lshl_u32", "v_cndmask_b32_e64")


def tool(name):
    for d in (os.environ.get("LLVM_BIN", ""), "/opt/rocm/llvm/bin", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")):
        p = os.path.join(d, name)
        if d and os.path.exists(p):
            return p
    return shutil.which(name)


def disassemble(lib):
    """llvm-objdump -d of the first gfx950 code object of the library (core.hip's: the NTT pass kernels)."""
    objcopy, bundler, objdump = tool("llvm-objcopy"), tool("clang-offload-bundler"), tool("llvm-objdump")
    if not (objcopy and bundler and objdump):
        raise FileNotFoundError("llvm-objcopy / clang-offload-bundler / llvm-objdump not found")
    with tempfile.TemporaryDirectory() as td:
        fat, co = os.path.join(td, "fatbin"), os.path.join(td, "dev.co")
        subprocess.check_call([objcopy, "--dump-section=.hip_fatbin=" + fat, lib, os.path.join(td, "copy.so")])
        subprocess.check_call([bundler, "--type=o", "--input=" + fat, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co, "--unbundle"])
        return subprocess.check_output([objdump, "-d", co], text=True)


def kernels(text):
    """{(LR, LC): [mnemonic + operands, ...]} of every fixed8 instantiation."""
    out, cur = {}, None
    for line in text.splitlines():
        m = KERNEL_RE.match(line)
        if m:
            cur = out.setdefault((int(m.group(2)), int(m.group(3))), [])
            continue
        if re.match(r"^[0-9a-f]+ <", line):
            cur = None
            continue
        if cur is not None:
            ins = line.split("//")[0].strip()
            if ins:
                cur.append(ins)
    return out


def classify(ins):
    op = ins.split()[0]
    if op.startswith("s_nop"):
        return "s_nop"
    if op.startswith("scratch_"):
        return "scratch"
    if not op.startswith("v_"):
        return None
    if op in FIELD and ("s[" in ins or "vcc" in ins):
        # a select or an add that only builds an index (no SGPR-pair carry / mask operand) is not field arithmetic
        return "field"
    if op.startswith(B_OTHER_PREFIX):
        return "b_other"
    return "a"


def counts(body):
    c = {"field": 0, "b_other": 0, "a": 0, "s_nop": 0, "s_nop_0": 0, "s_nop_1": 0, "scratch": 0, "g_vaddr": 0, "g_saddr": 0, "st_vaddr": 0,
         "total": len(body)}
    for ins in body:
        if ins.startswith("global_"):
            vaddr = ins.rstrip().endswith("off")
            c["g_vaddr" if vaddr else "g_saddr"] += 1
            c["st_vaddr"] += vaddr and ins.startswith("global_store")
        k = classify(ins)
        if k:
            c[k] += 1
        if k == "s_nop":
            c["s_nop_0" if ins.split()[1] == "0" else "s_nop_1"] += 1
    return c


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", default=os.path.join(REPO, "stark-anatomy_amd", "libstarkcore.so"))
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    ks = kernels(disassemble(a.lib))
    if not ks:
        sys.exit("no ntt_pass_kernel_fixed8 in " + a.lib)
    res = {"%d,%d" % k: counts(v) for k, v in sorted(ks.items())}
    if a.json:
        print(json.dumps(res, indent=1))
        return
    cols = ("total", "field", "b_other", "a", "s_nop", "s_nop_0", "s_nop_1", "scratch", "g_vaddr", "g_saddr", "st_vaddr")
    print("%-14s" % "fixed8<LR,LC>" + "".join("%9s" % c for c in cols))
    for k, c in res.items():
        print("%-14s" % ("<" + k + ">") + "".join("%9d" % c[x] for x in cols))


if __name__ == "__main__":
    main()
