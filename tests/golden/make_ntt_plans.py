#!/usr/bin/env python3
"""Fixture of the NTT planner's output: SHA-256 of each case of tests/emu/plan_dump.cpp built against a csrc/ directory.

The fixture pins the plans of a known-good planner, so that a rewrite of csrc/ntt_plan.h can be shown to plan every case
identically (tests/test_ntt_plans.py).  Generate it from the csrc/ of the commit whose plans are the reference, e.g.

    git archive <commit> stark-anatomy_amd/csrc | tar -x -C /tmp/ref
    python tests/golden/make_ntt_plans.py --csrc /tmp/ref/stark-anatomy_amd/csrc [--dump /tmp/ref_plans.txt]

--dump also writes the full dump, to diff against the one a failing test prints.
"""
import argparse
import hashlib
import json
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
SRC = os.path.join(REPO, "tests", "emu", "plan_dump.cpp")
FIXTURE = os.path.join(HERE, "ntt_plans.json")


def dump(csrc, cxx_flags=("-O2",)):
    """Build plan_dump.cpp against `csrc` and return {case name: dump text}, in the harness's order."""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "plan_dump")
        subprocess.check_call(["g++", *cxx_flags, "-std=c++17", "-I", csrc, "-o", exe, SRC])
        text = subprocess.run([exe], check=True, stdout=subprocess.PIPE).stdout.decode()
    cases = {}
    for block in text.split("case ")[1:]:
        name, _, body = block.partition("\n")
        cases[name] = body
    return cases


def digests(cases):
    return {name: hashlib.sha256(body.encode()).hexdigest() for name, body in cases.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--csrc", default=os.path.join(REPO, "stark-anatomy_amd", "csrc"), help="directory holding ntt_plan.h")
    ap.add_argument("--out", default=FIXTURE)
    ap.add_argument("--dump", help="also write the full dump here")
    a = ap.parse_args()
    cases = dump(os.path.abspath(a.csrc))
    if a.dump:
        with open(a.dump, "w") as f:
            f.writelines(f"case {name}\n{body}" for name, body in cases.items())
    with open(a.out, "w") as f:
        json.dump(digests(cases), f, indent=0)
        f.write("\n")
    print(f"{len(cases)} cases -> {a.out}")


if __name__ == "__main__":
    main()
