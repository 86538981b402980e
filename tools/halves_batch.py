#!/usr/bin/env python3
"""The data-dependent worst case of the eight-element batch kernels: 64 columns of 2^20 whose first half is 0 and second half 1
(u - v = -1 in the first butterflies of every tile of the forward transform's first pass), forward + inverse per step, against the
same batch of random columns.  Prints G elements / s (best of 3 x 100 steps) and whether the round trip is exact.

  python3 tools/halves_batch.py [--tune fast_fixups=0]"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "stark-anatomy_amd"), REPO, os.path.join(REPO, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tune", action="append", default=[])
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--columns", type=int, default=64)
    args = ap.parse_args()
    import torch
    import starkcore as sc
    from oracle import py_oracle as po
    sc.init()
    for kv in args.tune:
        k, v = kv.split("=")
        sc.set_tuning(k, int(v))
    n, cols = 1 << args.log2n, args.columns
    rt = sc.fe_bytes(po.primitive_nth_root(n))
    dev = torch.device("cuda", 0)
    halves = torch.zeros((cols, n, 2), dtype=torch.int64, device=dev)
    halves[:, n // 2:, 0] = 1
    g = torch.Generator(device="cuda:0")
    g.manual_seed(20)
    rand = torch.randint(0, 1 << 62, (cols, n, 2), dtype=torch.int64, device=dev, generator=g)
    for name, x in (("0/1 halves", halves), ("random", rand)):
        y, z = torch.empty_like(x), torch.empty_like(x)
        best = None
        for rep in range(4):            # the first repetition warms up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(100):
                sc._check(sc.lib().sc_ntt_columns_dev(x.data_ptr(), y.data_ptr(), n, cols, rt, 0, None))
                sc._check(sc.lib().sc_ntt_columns_dev(y.data_ptr(), z.data_ptr(), n, cols, rt, 1, None))
            sc.synchronize()
            dt = (time.perf_counter() - t0) / 100
            if rep and (best is None or dt < best):
                best = dt
        print("%s batch 2^%d x %d fwd+inv: %.3f G el/s (best of 3 x 100 steps), roundtrip exact %s" % (name, args.log2n, cols, 2 * n * cols / best / 1e9, bool(torch.equal(z, x))))


if __name__ == "__main__":
    main()
