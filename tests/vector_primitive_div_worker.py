"""sc_pointwise_div_dev against a * b^-1 in Python integers, for tests/test_gpu_vector_primitives.py -- which imports the checks below
for the default pointwise_div_kernel<16> and starts this file as a fresh process with STARKCORE_DIV_K=8 for pointwise_div_kernel<8>
(the constant is read once per process).  As a program it runs the K = 8 shapes and one zero-divisor case of
tests/vector_primitive_cases.py and ends at the first failure with a non-zero exit status."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), os.path.join(REPO, "stark-anatomy_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

import vector_primitive_cases as vc

SC_ERR_DIV_ZERO = -5


def dev(sc, vals, guard=1):
    """the values on the device with `guard` sentinel elements behind them"""
    return sc.DeviceVector.from_bytes(vc.pack(vals) + vc.SENTINEL * guard)


def blank(sc, n, guard=1):
    return sc.DeviceVector.from_bytes(vc.SENTINEL * (n + guard))


def read(vec, n):
    """the first n elements; what lies behind them must still be the sentinel"""
    raw = vec.to_bytes()
    assert raw[16 * n:] == vc.SENTINEL * (vec.n - n), "written past the stated length"
    return vc.unpack(raw[:16 * n])


def check_quotients(sc, n):
    """out of place, d_out == d_a and d_out == d_b"""
    lib = sc.lib()
    a, b = vc.div_operands(n)
    want = vc.div_expected(n)
    for alias in ("none", "a", "b"):
        da, db = dev(sc, a), dev(sc, b)
        out = {"none": blank(sc, n), "a": da, "b": db}[alias]
        assert lib.sc_pointwise_div_dev(da.ptr, db.ptr, out.ptr, n, None) == 0, (n, alias)
        assert read(out, n) == want, (n, alias)
        if alias != "a":
            assert read(da, n) == list(a), (n, alias)
        if alias != "b":
            assert read(db, n) == list(b), (n, alias)


def check_zero_divisor(sc, n, K, place):
    """one zero divisor: SC_ERR_DIV_ZERO; only the quotients that share its thread's inversion (K per thread) are spoiled; and the next
    call, on clean operands, succeeds -- the flag word was cleared"""
    lib = sc.lib()
    a, b = vc.div_operands(n)
    want = vc.div_expected(n)
    bz = list(b)
    bz[place] = 0
    da, db, out = dev(sc, a), dev(sc, bz), blank(sc, n)
    assert lib.sc_pointwise_div_dev(da.ptr, db.ptr, out.ptr, n, None) == SC_ERR_DIV_ZERO, (n, place)
    got = read(out, n)
    spoiled = {i for i in range(n) if got[i] != want[i]}
    assert spoiled <= vc.div_companions(n, K, place), (n, K, place, sorted(spoiled)[:20])
    dc = dev(sc, b)
    assert lib.sc_pointwise_div_dev(da.ptr, dc.ptr, out.ptr, n, None) == 0, (n, place)
    assert read(out, n) == want, (n, place)


def main():
    assert os.environ.get("STARKCORE_DIV_K") == "8"
    import starkcore as sc
    assert sc.device_count() > 0, "no GPU visible"
    sc.init()
    for n in vc.DIV_SIZES[8]:
        check_quotients(sc, n)
    for n in vc.DIV_ZERO_SIZES[8]:
        # with sixteen divisors per thread the companions of element 0 would be 0, 256, 512, ...: the subset below holds for K = 8 only
        assert vc.div_companions(n, 8, 0) < vc.div_companions(n, 16, 0)
        for place in vc.div_zero_places(n):
            check_zero_divisor(sc, n, 8, place)
    print("ok: pointwise_div_kernel<8> at n = %s" % (vc.DIV_SIZES[8],))


if __name__ == "__main__":
    main()
