"""Cases of the randomized trace matrix of a batch (sc_randomized_columns_dev, randomized_cols_thread of csrc/columns.cuh), shared by
the CPU walk (tests/test_randomize_emu.py) and the GPU test (tests/test_gpu_randomized_columns.py).  The reference is Python's own
`int.from_bytes(b, "big") % p` -- Field.sample (code/algebra.py:116-120) -- and plain list copies."""
import random

P = 1 + 407 * (1 << 119)
SENTINEL = (1 << 128) - 1            # not a residue: the kernel cannot produce it

WIDTHS = [1, 16, 17, 32]
# (members, registers, rows, extra): one element; several members and registers; a column of 557 elements -- three workgroups of
# 256 threads, the last one partial, the trace ending inside the second
SHAPES = [(1, 1, 0, 1), (3, 2, 28, 5), (2, 3, 300, 257)]
# (ld_trace - rows, ld_out - (rows + extra), draws_stride - extra * registers * width)
PADDINGS = [(0, 0, 0), (3, 5, 7)]


def special_draws(width):
    """draws whose integer is at or above p in one or both 128-bit halves: all 0xFF bytes, p itself, 2^128 - 1 (where they fit)"""
    out = [b"\xff" * width]
    if width >= 16:
        out += [P.to_bytes(width, "big"), ((1 << 128) - 1).to_bytes(width, "big")]
    if width >= 17:
        out += [(P << 8 * (width - 16)).to_bytes(width, "big") if width < 32 else (P << 128 | P).to_bytes(32, "big")]
    return out


def pack(values):
    return b"".join(v.to_bytes(16, "little") for v in values)


def unpack(raw):
    return [int.from_bytes(raw[i:i + 16], "little") for i in range(0, len(raw), 16)]


class Case:
    """one call: the arguments as buffers, and what the output matrix must hold afterwards (sentinels in its padding)"""

    def __init__(self, shape, width, padding, seed=0):
        self.members, self.registers, self.rows, self.extra = shape
        self.width = width
        pad_trace, pad_out, pad_draws = padding
        rng = random.Random(hash((shape, width, padding, seed)) & 0xFFFFFFFF)
        members, registers, rows, extra = shape
        cols = members * registers
        self.ld_trace, self.ld_out = rows + pad_trace, rows + extra + pad_out
        block = extra * registers * width
        self.draws_stride = block + pad_draws
        columns = [[rng.randrange(P) for _ in range(rows)] for _ in range(cols)]
        if rows:
            columns[0][0], columns[-1][-1] = 0, P - 1
        self.trace = b"".join(pack(column + [SENTINEL] * pad_trace) for column in columns)
        per_member = []
        for m in range(members):
            draws = [bytes(rng.getrandbits(8) for _ in range(width)) for _ in range(extra * registers)]
            per_member.append(draws)
        specials = special_draws(width)
        for k, draw in enumerate(specials):                  # the first draws of member 0 and the last of the last member
            per_member[0][k % len(per_member[0])] = draw
            per_member[-1][-1 - k % len(per_member[-1])] = draw
        self.draws = b"".join(b"".join(draws) + b"\xa5" * pad_draws for draws in per_member)
        self.want = []
        for m in range(members):
            for s in range(registers):
                tail = [int.from_bytes(per_member[m][r * registers + s], "big") % P for r in range(extra)]
                self.want += columns[m * registers + s] + tail + [SENTINEL] * pad_out
        self.cols = cols

    def blank_output(self):
        return pack([SENTINEL] * (self.cols * self.ld_out))


def all_cases():
    return [(shape, width, padding) for shape in SHAPES for width in WIDTHS for padding in PADDINGS]


def case_id(case):
    shape, width, padding = case
    return "%dx%dx%d+%d-w%d-%s" % (*shape, width, "padded" if any(padding) else "tight")
