#!/usr/bin/env python3
"""Golden vectors of the tutorial's signature scheme, from the reference's FastRPSSS (code/fast_rpsss.py).

Runs ONLY where the reference's code/ directory is on disk (its path is the first argument, or REFERENCE_CODE); the GPU box never
runs this.  os.urandom is replaced by the seeded stand-in the package's tests and tools/verify_timing.py use (random.Random(seed),
one getrandbits(8) per byte), installed after FastRPSSS() is constructed.  Then: 8 consecutive keygen() calls, and sign(sk of the
first pair, DOCUMENT) drawing from the same stream.  Written to rpsss.json next to this file: the seed, the key pairs, the document,
and the signature's length and SHA-256 (the signature itself is about 1.3 MB).  Only DATA is written.  The reference's sign takes
about 40 s; its verify is not run.

usage:  python tests/golden/make_rpsss_golden.py /path/to/reference/code
"""
import hashlib
import json
import os
import random
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REFERENCE_CODE", "")
assert REF and os.path.isdir(REF), "usage: make_rpsss_golden.py REFERENCE_CODE_DIR"
REF = os.path.abspath(REF)
sys.path.insert(0, REF)              # ONLY the reference: the package has modules of the same names (rescue_prime, fast_stark, ...)
sys.setrecursionlimit(10000)

import rescue_prime as ref_rescue_prime  # noqa: E402  (reference)
import fast_rpsss as ref_fast_rpsss      # noqa: E402

for mod in (ref_rescue_prime, ref_fast_rpsss, sys.modules["fast_stark"], sys.modules["algebra"]):
    assert os.path.abspath(mod.__file__).startswith(REF), mod.__file__

SEED = 20261016
KEYS = 8
DOCUMENT = b"Rescue-Prime STARK signatures on the MI355X"

rpsss = ref_fast_rpsss.FastRPSSS()
rng = random.Random(SEED)
os.urandom = lambda k: bytes(rng.getrandbits(8) for _ in range(k))
pairs = [rpsss.keygen() for _ in range(KEYS)]
t0 = time.time()
signature = rpsss.sign(pairs[0][0], DOCUMENT)
print("reference sign: %.1f s, %d bytes" % (time.time() - t0, len(signature)))
out = {
    "seed": SEED,
    "keys": [[str(sk.value), str(pk.value)] for sk, pk in pairs],
    "document": DOCUMENT.decode(),
    "signed_key": 0,
    "signature_len": len(signature),
    "signature_sha256": hashlib.sha256(signature).hexdigest(),
}
with open(os.path.join(HERE, "rpsss.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
