"""Hand-built rows for TSDBHIP_DESC_QUALS_PROVEN (test_desc_certify_cpu.py,
test_values_only_certificate.py): a row's qualifiers as host-order 16-bit words, each
(delta << 4) | flags, with what the statement says of the row.

The statement: a row of n >= 2 cells is proven iff, with q0 and q1 its first
two words, q1 - q0 is positive and a multiple of 16, q0 + (n - 1) (q1 - q0)
does not exceed 0xFFFF, and word c is q0 + c (q1 - q0) for every c. A row of
one cell is proven."""
import numpy as np

from opentsdb_amd import packing, synth

I8 = 0x7  # flags of an 8-byte integer cell


def quals(n, d0=0, step=1, flags=I8):
    """words of n cells at deltas d0, d0 + step, ... (mod 2^16: a delta past
    4095 wraps, as the bytes of such a row would have to)"""
    return ((((d0 + step * np.arange(n, dtype=np.int64)) << 4) | flags) & 0xFFFF).astype(np.uint16)


def changed(q, cell, fn):
    q = q.copy()
    q[cell] = fn(int(q[cell])) & 0xFFFF
    return q


# what a single bad cell can be: the flags nibble, or the delta
FLAGS = {"float-flag": lambda q: q | 0x8, "width-4": lambda q: (q & ~0x7) | 0x3, "width-5": lambda q: (q & ~0x7) | 0x4}
DELTA = {"delta+1": lambda q: q + 16}


def places(n):
    """cell 1, cell 2, a middle cell, the last cell"""
    return sorted({1, 2, n // 2, n - 1})


def hand_rows():
    """[(name, words, proven)]"""
    rows = [
        ("one cell", quals(1, 17), True),
        ("two cells", quals(2, 5, 3), True),
        ("two cells, delta 4095 exactly", quals(2, 0, 4095), True),
        ("4096 cells, the last at delta 4095", quals(4096), True),
        ("float cells on one step", quals(40, 3, 2, flags=0xB), True),
        ("4097 cells: delta 4096", quals(4097), False),
        ("three cells: delta 2047 + 2 x 2048", quals(3, 2047, 2048), False),
        ("step 0", quals(3, 9, 0), False),
        ("step 0, two cells", quals(2, 9, 0), False),
        ("a falling step", quals(3, 10, -5), False),
        ("a falling step, two cells", quals(2, 10, -5), False),
    ]
    base = quals(20, 4, 2)
    for kind in (FLAGS, DELTA):
        for what, fn in kind.items():
            for c in places(len(base)):
                rows.append((f"{what} at cell {c} of 20", changed(base, c, fn), False))
    return rows


def kv(words, base_time=synth.T0, value=0):
    """a compacted row of 8-byte cells with these qualifier words (the values
    only have to be as long as an 8-byte row's: the statement is about the
    qualifiers)"""
    n = len(words)
    qb = np.asarray(words, ">u2").tobytes()
    vb = int(value).to_bytes(8, "big", signed=True) * n + (b"\x00" if n > 1 else b"")
    return packing.KeyValue(base_time, qb, vb)


def table(rows):
    """one span a row"""
    return packing.pack_spans([[kv(w)] for w in rows])
