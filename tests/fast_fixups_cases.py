"""Inputs that raise the tile flag of the eight-element batch kernels (ntt_pass_kernel_fixed8 / ntt_pass_redo8_kernel, csrc/core.hip)
exactly where a case wants it -- one lane of one tile of one pass, a late round, a product -- shared by the CPU test that proves they
do (test_fast_fixups_cases_emu.py) and the device test that runs them (test_gpu_fast_fixups_sparse.py).

Construction.  The device flag of every top-limb form equals its portable twin's lane by lane (test_gpu_field_pairs.py), so the CPU
emulation (tests/emu/ntt_fast_emu.cpp: fx_*) predicts which workgroups a launch marks.  A pass, and every round of a tile, is an
invertible linear map and the whole transform has an exact inverse in the oracle: a case chooses the state where it wants the flag
-- the input of a pass, or the LDS image of one tile at the input of a round, with seeded random values everywhere else, the other
tiles' outputs included --, pushes it forward through the exact emulated rounds and passes to the transform's output y, and takes
x = (inverse transform of y) from the oracle.  The transform of x then meets the chosen state at that place.

Which elements meet where is asked of the kernels' own code, never re-derived: fx_tile_map gives the positions a lane's eight elements
come from in a round (Round::setup / in_index / lds_index), fx_tile_store the positions it stores to and the direct-table entries it
multiplies by (scatter_global, load_twd).  Which two of a lane's elements meet in the first stage, and which entry of the tile's LDS
twiddle image that butterfly multiplies by, is found by search: plant, run the FAST emulation of that one round of that one tile,
keep the candidate that raises the flag in that round and that wave (3 runs for a pair, at most 2^(logR-1) for a twiddle).

Plants.  sub: (u, v) = (0, 1), u - v borrows and limb 0 wraps.  add: (p-1, 2^32).  Product d * w with a Montgomery-form table value w:
the exact result r = d w 2^-128 is chosen as a multiple of 2^32 (in the spirit of field_cases.flagged_products), d = r 2^128 / w, and
the first such r for which field_cases.model("mul", d, w) flags is kept (about every second one).  At a butterfly u is the random
background value and v = u - d, with model("add") and model("sub") of (u, v) clear; at the store the chosen state is the pass's
output, whose element is r itself.

Shapes: A = 2^17 x 8, passes (9,3) then (8,4); B = 2^19 x 2, passes (10,2) then (9,3): all three SC_FIXED8_SHAPES, the smallest
launches that take them.  Cases, for A and B, forward and inverse: p0-sub, p0-add-last, p1-sub, late (A: last round of pass 0,
B: last round of pass 1), mul-bfly (round 0 of pass 0), mul-store (the direct four-step table of pass 0, the one scaled by n^-1 for an
inverse) and three (workgroups 0, last and one that xcd_remap moves, all in pass 1, and a store product in one tile of pass 0).

Left out, because the default plans never execute the site under FAST (fx_info says which kernel a pass takes):
  * 2^22 x 2 (`first-pass`, `last-pass`): three passes of 2^11-element tiles -- (8,3), (7,4), (7,4) with four elements a thread; the
    eight-element kernels serve 2^12-element tiles only, so no pass of that plan has a flag at all;
  * finish_global's twiddle on load: tw_on_load defaults to 0, PassParams::twd_in is null in every plan;
  * P.scale at the store: set only for a single-pass inverse (n <= 2^11); the two-pass inverses fold n^-1 into pass 0's direct table,
    which mul-store covers.

Generation time on one CPU core (measured), the builder's two checks -- the FAST and the exact emulation of both passes, 0.8 s --
included: 1.0-1.5 s for the cases planted in the input (p0-sub, p0-add-last, mul-bfly), 2.3-3.1 s for those planted behind pass 0
(p1-sub, late, mul-store, three), which add the exact passes up to y and the oracle's inverse of every column; A and B alike.

Seen while building these: a 2^32 planted in pass 1's input is a multiple of 2^32 at pass 0's store and may flag that product too
(`three` plants (0, 1) only), and the constant and alternating inputs of test_gpu_fast_fixups.py are not flag-free: p-1 flags every
tile of pass 0, and the inverse of either flags one tile a column in pass 1.
"""
import collections
import ctypes
import functools
import os
import subprocess

import numpy as np

import field_cases as fc
import synth
from oracle import py_oracle as po

P, R = fc.P, fc.R
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(REPO, "tests", "emu")
SHAPES = {"A": (17, 8), "B": (19, 2)}
NAMES = ("p0-sub", "p0-add-last", "p1-sub", "late", "mul-bfly", "mul-store", "three")
SUB, ADD = (0, 1), (P - 1, 1 << 32)


def case_ids():
    return [(s, inv, name) for s in SHAPES for inv in (0, 1) for name in NAMES]


@functools.lru_cache(maxsize=None)
def load_emu():
    """tests/emu/libntt_fast_emu.so, built on demand exactly as test_fast_fixups_emu.py builds it"""
    so = os.path.join(EMU_DIR, "libntt_fast_emu.so")
    srcs = [os.path.join(EMU_DIR, f) for f in ("ntt_fast_emu.cpp", "ntt_emu.cpp")] + \
           [os.path.join(REPO, "stark-anatomy_amd", "csrc", f) for f in ("field.cuh", "ntt_tile.cuh", "ntt_plan.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, srcs[0]])
    lib = ctypes.CDLL(so)
    vp, i32, u32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32
    lib.fx_open.restype = vp
    lib.fx_open.argtypes = [i32, i32, vp, i32]
    lib.fx_close.restype = None
    lib.fx_close.argtypes = [vp]
    lib.fx_info.restype = None
    lib.fx_info.argtypes = [vp, vp]
    lib.fx_grid_tile.restype = u32
    lib.fx_grid_tile.argtypes = [vp, i32, u32, i32]
    lib.fx_pass.restype = i32
    lib.fx_pass.argtypes = [vp, i32, i32, vp, vp, vp, vp]
    lib.fx_tile.restype = i32
    lib.fx_tile.argtypes = [vp, i32, u32, i32, i32, i32, vp, vp, vp, vp]
    lib.fx_tile_map.restype = i32
    lib.fx_tile_map.argtypes = [vp, i32, u32, i32, vp]
    lib.fx_tile_store.restype = i32
    lib.fx_tile_store.argtypes = [vp, i32, u32, vp, vp, vp, vp, vp]
    return lib


def fe_get(a, i):
    return int(a[i, 0]) | (int(a[i, 1]) << 64)


def fe_set(a, i, v):
    a[i, 0] = v & ((1 << 64) - 1)
    a[i, 1] = v >> 64


def background(seed, salt, count):
    """seeded canonical values; streams of different (seed, salt) do not overlap"""
    return synth.synth_packed((seed << 40) + (salt << 33), count)


def _ptr(a):
    return None if a is None else a.ctypes.data


Pass = collections.namedtuple("Pass", "logR logC loge ntiles threads rounds fixed8 fast")


class Plan:
    """the emulation's plan of `cols` columns of 2^logn, planned as sc_ntt_columns_dev plans them"""

    def __init__(self, logn, cols, inverse):
        self.lib = load_emu()
        self.logn, self.cols, self.inverse, self.n = logn, cols, inverse, 1 << logn
        self.root = po.primitive_nth_root(self.n)
        self.h = self.lib.fx_open(logn, cols, int(self.root).to_bytes(16, "little"), inverse)
        assert self.h, "no plan"
        info = (ctypes.c_int * 40)()
        self.lib.fx_info(self.h, info)
        self.passes = [Pass(*info[1 + 8 * i:9 + 8 * i]) for i in range(info[0])]
        self.count = self.n * cols

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.fx_close(self.h)
            self.h = None

    def nwg(self, k):
        return self.passes[k].ntiles * self.cols

    def grid_tile(self, k, wg, remap=1):
        return self.lib.fx_grid_tile(self.h, k, wg, remap)

    def empty(self):
        return np.zeros((self.count, 2), dtype=np.uint64)

    def run_pass(self, k, buf, fast=True, exact=True, remap=1):
        """(FAST output or None, exact output or None, words per workgroup or None) of pass k on its input `buf`"""
        of = self.empty() if fast and self.passes[k].fast else None
        oe = self.empty() if exact else None
        words = np.zeros(self.nwg(k), dtype=np.uint32) if of is not None else None
        rc = self.lib.fx_pass(self.h, k, remap, _ptr(buf), _ptr(of), _ptr(oe), _ptr(words))
        assert rc == (1 if self.passes[k].fast else 0), rc
        return of, oe, words

    def tile(self, k, tile, r0, r1, fast, inp=None, state=None, out=None):
        word = ctypes.c_uint32(0)
        rc = self.lib.fx_tile(self.h, k, tile, r0, r1, int(fast), _ptr(inp), _ptr(state), _ptr(out), ctypes.byref(word))
        assert rc == self.passes[k].rounds, rc
        return word.value

    def tile_map(self, k, tile, r):
        pos = np.zeros((self.passes[k].threads, 8), dtype=np.uint64)
        assert self.lib.fx_tile_map(self.h, k, tile, r, _ptr(pos)) == 0
        return pos

    @functools.lru_cache(maxsize=8)
    def tile_store(self, k, tile):
        """(kind bits, store positions [threads][8], direct-table entries [threads * 8][2], scale, LDS twiddle image [R/2][2])"""
        pk = self.passes[k]
        scratch = self.empty()
        pos = np.zeros((pk.threads, 8), dtype=np.uint64)
        twd = np.zeros((pk.threads * 8, 2), dtype=np.uint64)
        scale = np.zeros((1, 2), dtype=np.uint64)
        img = np.zeros((1 << (pk.logR - 1), 2), dtype=np.uint64)
        kind = self.lib.fx_tile_store(self.h, k, tile, _ptr(scratch), _ptr(pos), _ptr(twd), _ptr(scale), _ptr(img))
        assert kind >= 0 and not scratch.any()
        assert len(set(pos.ravel().tolist())) == pk.threads * 8
        return kind, pos, twd, fe_get(scale, 0), img

    def oracle(self, data):
        """the transform of every column, from the C oracle"""
        f = po.C.intt if self.inverse else po.C.ntt
        return b"".join(f(self.root, data[16 * self.n * c:16 * self.n * (c + 1)], self.n) for c in range(self.cols))

    def oracle_inverse(self, data):
        f = po.C.ntt if self.inverse else po.C.intt
        return b"".join(f(self.root, data[16 * self.n * c:16 * self.n * (c + 1)], self.n) for c in range(self.cols))


def word_of(waves, rnd):
    return sum(1 << w for w in waves) | ((rnd + 1) << 8)


# one planted flag: workgroup `grid` (under the default xcd_remap) = tile `tile` of pass `k`, the waves and the first round that flag
Flag = collections.namedtuple("Flag", "k grid tile waves round")
# what a case chose, for the CPU test: ("buffer", k, array) = the input of pass k; ("lds", k, tile, round, array) = a tile's LDS image
Case = collections.namedtuple("Case", "shape name logn cols inverse seed data flagged chosen plan")


class _BackgroundFlag(Exception):
    pass


def _candidates():
    k = 0
    while True:
        k += 1
        r = (k * 0x9E3779B97F4A7C15F39CC060 % (1 << 96)) << 32          # (a 96-bit multiplier: the results spread over [0, 2^128) from k = 1 on)
        if 0 < r < P:
            yield r


def flagged_product(w_m, ok=lambda d: True):
    """(d, r): d * w_m * 2^-128 = r, a multiple of 2^32, with the product's top-limb correction flagged in the model"""
    winv = pow(w_m, -1, P)
    for r in _candidates():
        d = r * R % P * winv % P
        flag, exact = fc.model("mul", d, w_m)
        if flag and ok(d):
            assert exact == r
            return d, r
    raise AssertionError("unreachable")


class _Builder:
    def __init__(self, plan, seed):
        self.plan, self.seed, self.salt = plan, seed, 0
        self.scratch = plan.empty()
        self.lds0 = np.zeros((1 << 12, 2), dtype=np.uint64)      # receives the LDS image a partial run leaves
        self.flags, self.chosen = [], []

    def bg(self, count):
        self.salt += 1
        return background(self.seed, self.salt, count)

    def first_stage_pair(self, k, tile, r, tid, buf):
        """the positions of the two elements of lane `tid` that meet in the first stage of round r: searched with (0, 1) planted
        into `buf` (the pass's input for r = 0, the tile's LDS image otherwise), which is left as it was"""
        plan, pk = self.plan, self.plan.passes[k]
        pos = plan.tile_map(k, tile, r)[tid]
        want = word_of([tid >> 6], r)
        found = []
        for a, b in ((0, 4), (0, 2), (0, 1)):
            pa, pb = int(pos[a]), int(pos[b])
            keep = buf[[pa, pb]].copy()
            fe_set(buf, pa, 0)
            fe_set(buf, pb, 1)
            state = self.lds0.copy() if r == 0 else buf.copy()
            w = plan.tile(k, tile, r, r + 1, True, inp=buf if r == 0 else None, state=state, out=self.scratch if r + 1 == pk.rounds else None)
            buf[[pa, pb]] = keep
            if w == want:
                found.append((pa, pb))
        assert len(found) == 1, (k, tile, r, tid, found)
        return found[0]

    def plant_pair(self, k, wg, r, tid, buf, values):
        tile = self.plan.grid_tile(k, wg)
        pa, pb = self.first_stage_pair(k, tile, r, tid, buf)
        fe_set(buf, pa, values[0])
        fe_set(buf, pb, values[1])
        self.flags.append(Flag(k, wg, tile, (tid >> 6,), r))
        return tile

    def plant_butterfly_product(self, k, wg, r, tid, buf):
        """u stays, v = u - d with d * (the butterfly's twiddle) flagged: the twiddle is searched in the tile's LDS image"""
        plan, pk = self.plan, self.plan.passes[k]
        tile = plan.grid_tile(k, wg)
        pa, pb = self.first_stage_pair(k, tile, r, tid, buf)
        u, keep = fe_get(buf, pa), fe_get(buf, pb)
        img = plan.tile_store(k, tile)[4]
        want = word_of([tid >> 6], r)
        tried = 0
        for e in range(len(img)):
            w_m = fe_get(img, e)
            if w_m == fc.R_M:
                continue                        # w^0: a product the kernel still computes in this round, but not a real twiddle
            d, _ = flagged_product(w_m, ok=lambda d: not fc.model("sub", u, (u - d) % P)[0] and not fc.model("add", u, (u - d) % P)[0])
            fe_set(buf, pb, (u - d) % P)
            state = self.lds0.copy() if r == 0 else buf.copy()
            tried += 1
            if plan.tile(k, tile, r, r + 1, True, inp=buf if r == 0 else None, state=state, out=self.scratch if r + 1 == pk.rounds else None) == want:
                self.flags.append(Flag(k, wg, tile, (tid >> 6,), r))
                return tile
        fe_set(buf, pb, keep)
        raise AssertionError(("no twiddle of the image flags", k, tile, r, tid, tried))

    def plant_store_product(self, k, wg, tid, i, out_buf):
        """element i of lane tid of the tile's stores: the pass's output there is r, the product (r 2^128 / t) * t flagged"""
        plan, pk = self.plan, self.plan.passes[k]
        tile = plan.grid_tile(k, wg)
        kind, pos, twd, _, _ = plan.tile_store(k, tile)
        assert kind == 1, kind                  # a direct table at the store, no final scale
        _, r = flagged_product(fe_get(twd, tid * 8 + i))
        fe_set(out_buf, int(pos[tid, i]), r)
        self.flags.append(Flag(k, wg, tile, (tid >> 6,), pk.rounds - 1))
        return tile


def _interior(plan, k, moved=False):
    """a workgroup strictly inside the grid of pass k, not in column 0; moved: one whose tile differs from its index under xcd_remap"""
    nwg = plan.nwg(k)
    for wg in range(nwg // 2 + 3, nwg - 1):
        if not moved or plan.grid_tile(k, wg) != wg:
            return wg
    raise AssertionError("no such workgroup")


def _construct(shape, inverse, name, seed):
    logn, cols = SHAPES[shape]
    plan = Plan(logn, cols, inverse)
    assert len(plan.passes) == 2 and all(p.fast and p.threads == 512 for p in plan.passes), plan.passes
    b = _Builder(plan, seed)
    last_tid = 511 - 9                           # a lane of the last wave
    if name in ("p0-sub", "p0-add-last", "mul-bfly"):
        at, buf = 0, b.bg(plan.count)
        if name == "p0-sub":
            b.plant_pair(0, _interior(plan, 0), 0, 64 * 3 + 21, buf, SUB)
        elif name == "p0-add-last":
            b.plant_pair(0, plan.nwg(0) - 1, 0, last_tid, buf, ADD)
        else:
            b.plant_butterfly_product(0, _interior(plan, 0), 0, 64 * 5 + 40, buf)
        b.chosen.append(("buffer", 0, buf.copy()))
    elif name in ("p1-sub", "mul-store", "three"):
        at, buf = 1, b.bg(plan.count)
        if name == "p1-sub":
            b.plant_pair(1, _interior(plan, 1), 0, 64 * 2 + 5, buf, SUB)
        elif name == "mul-store":
            b.plant_store_product(0, _interior(plan, 0), 64 * 6 + 33, 5, buf)
        else:
            b.plant_pair(1, 0, 0, 7, buf, SUB)
            # (0, 1) here too: a 2^32 in pass 1's input is a multiple of 2^32 at pass 0's store, where the product may flag as well
            b.plant_pair(1, plan.nwg(1) - 1, 0, last_tid, buf, SUB)
            b.plant_pair(1, _interior(plan, 1, moved=True), 0, 64 * 4 + 63, buf, SUB)
            b.plant_store_product(0, _interior(plan, 0, moved=True), 64 + 2, 3, buf)
        b.chosen.append(("buffer", 1, buf.copy()))
    elif name == "late":
        k = 0 if shape == "A" else 1
        r = plan.passes[k].rounds - 1
        state = b.bg(1 << 12)
        wg = _interior(plan, k, moved=True)
        tile = b.plant_pair(k, wg, r, 64 * 6 + 11, state, SUB)
        at, buf = k + 1, b.bg(plan.count)        # the other tiles' outputs
        plan.tile(k, tile, r, r + 1, False, state=state.copy(), out=buf)
        b.chosen.append(("lds", k, tile, r, state))
    else:
        raise KeyError(name)
    if at == 0:
        data = buf.tobytes()
    else:
        for k in range(at, len(plan.passes)):
            buf = plan.run_pass(k, buf, fast=False)[1]
        data = plan.oracle_inverse(buf.tobytes())
    flagged = tuple(sorted(b.flags))
    assert len({(f.k, f.grid) for f in flagged}) == len(flagged)
    case = Case(shape, name, logn, cols, inverse, seed, data, flagged, b.chosen, plan)
    _check(case)
    return case


def emulate(case, remap=1):
    """the passes in turn, each on the exact output of the one before (what the redo leaves): [(FAST out, exact out, words)]"""
    buf = np.frombuffer(case.data, dtype=np.uint64).reshape(-1, 2)
    runs = []
    for k in range(len(case.plan.passes)):
        of, oe, words = case.plan.run_pass(k, buf, remap=remap)
        runs.append((of, oe, words))
        buf = oe
    return runs


def footprint(case, f):
    """the positions tile f.tile of pass f.k stores to"""
    return case.plan.tile_store(f.k, f.tile)[1].ravel().astype(np.int64)


def _check(case):
    """the builder's two checks: the FAST emulation of every pass flags exactly the planted workgroups (an extra flag of the random
    background, about 2^-32 per lane operation: _BackgroundFlag, the next seed), and in each of them FAST and exact outputs differ"""
    for k, (of, oe, words) in enumerate(emulate(case)):
        want = np.zeros_like(words)
        for f in case.flagged:
            if f.k == k:
                want[f.grid] = word_of(f.waves, f.round)
        if not np.array_equal(words, want):
            extra = [int(g) for g in np.nonzero(words)[0] if not want[g]]
            if extra and all(words[g] == want[g] for g in np.nonzero(want)[0]):
                raise _BackgroundFlag((k, extra))
            raise AssertionError((case.shape, case.name, case.inverse, k, [(int(g), hex(int(words[g])), hex(int(want[g]))) for g in np.nonzero(words != want)[0]]))
        rest = np.ones(len(of), dtype=bool)
        for f in case.flagged:
            if f.k == k:
                fp = footprint(case, f)
                assert not np.array_equal(of[fp], oe[fp]), f
                rest[fp] = False
        assert np.array_equal(of[rest], oe[rest]), k          # ... and nowhere else


@functools.lru_cache(maxsize=3)
def build(shape, inverse, name):
    """the case, deterministic: the first of the seeds 1, 2, 3 whose random background adds no flag of its own"""
    base = 1000 * (1 + list(SHAPES).index(shape)) + 100 * inverse + 10 * NAMES.index(name)
    for attempt in range(1, 4):
        try:
            return _construct(shape, inverse, name, base + attempt)
        except _BackgroundFlag:
            continue
    raise AssertionError(("the background flagged under three seeds: not chance", shape, inverse, name))
