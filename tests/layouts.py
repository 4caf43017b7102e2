"""Descriptor layouts other than the packer's (test_layouts_cpu.py,
test_layouts.py). packing.pack_spans lays every row out one way: qualifiers at
0 mod 8, values at 0 mod 16, rows in row order, gaps and tail zero.
tsdbhip_sg_desc allows far more (include/tsdbhip.h): rows anywhere inside the
buffers, in any order, at any value offset and any even qualifier offset, the
bytes outside rows never interpreted. `relayout` moves the rows of a SpanSet to
such a layout, byte for byte; LAYOUTS names the ones the tests run.

A layout is: the order of the rows inside the buffers, the qualifier residue
mod 8 and the value residue mod 16 (fixed, or cycling by row index), and the
fill byte of the lead before the first row, of every gap and of the tail. The
fill is 0xFF: a stray qualifier then reads 0xFFFF (delta 4095, flags 0xF), a
stray value -1 or NaN, and one misplaced cell shows in every aggregator (a
zero gap adds 0 to a sum and hides from min / max on one side)."""
import zlib
from dataclasses import dataclass

import numpy as np

from opentsdb_amd import packing

FILL = 0xFF
TAIL = 64  # fill bytes after the last row (>= 32; the device tests declare the buffers without them)
Q_UNIT, V_UNIT = 8, 16


@dataclass(frozen=True)
class Layout:
    name: str
    order: str = "asc"      # "asc" | "desc" | "perm": the rows' order inside the buffers
    q: tuple = (0,)         # qualifier residues mod 8, row r takes q[r % len(q)]; None: back to back
    v: tuple = (0,)         # value residues mod 16, likewise; None: cumulative value bytes + r
    fill: int = FILL
    odd: str = ""           # "q" | "v": row `odd_row` alone at residue 2 (q) / 8 (v)


LAYOUTS = {L.name: L for L in [
    Layout("packed", fill=0x00),                      # the control: the SpanSet itself
    Layout("poison"),                                 # the packer's residues; lead, gaps and tail poisoned
    Layout("shuffled", order="perm"),                 # offsets not monotone (what tsdbhip_desc_gather produces)
    Layout("reversed", order="desc"),                 # the last row at the lowest offset
    Layout("v8", v=(8,)),                             # W-aligned for 8-byte cells, not 16-aligned
    Layout("v4", v=(4,)),                             # W-aligned for 4-byte cells only
    Layout("v12", v=(12,)),
    Layout("vodd", v=(1, 7, 15)),                     # only the byte-wise loaders may take it
    Layout("q2", q=(2,)),                             # even, not 8-aligned qualifiers
    Layout("q4", q=(4,)),
    Layout("q6", q=(6,)),
    Layout("compact", q=None, v=None),                # tsdbhip_rows_out's placement: no lead, 1-byte value gaps
    Layout("mixed", order="perm", q=(0, 2, 4, 6), v=(0, 1, 4, 7, 8, 12, 15)),
    Layout("one_off_v", odd="v"),                     # `poison` except one row's values at 8 mod 16
    Layout("one_off_q", odd="q"),                     # `poison` except one row's qualifiers at 2 mod 8
]}
NAMES = list(LAYOUTS)


def _place(order, lens, res, unit, odd_row, odd_res):
    """offsets of the rows placed in `order`: a lead of one unit, then each row
    at the next offset of its residue that leaves a gap of at least one unit"""
    off = np.zeros(len(lens), np.uint64)
    pos = unit
    for r in order:
        want = odd_res if r == odd_row else res[r % len(res)]
        pos += (want - pos) % unit
        off[r] = pos
        pos += int(lens[r]) + unit
    return off, pos - unit if len(order) else 0


def row_order(n_rows, layout, seed=0):
    L = LAYOUTS[layout] if isinstance(layout, str) else layout
    if L.order == "asc":
        return list(range(n_rows))
    if L.order == "desc":
        return list(range(n_rows - 1, -1, -1))
    return [int(r) for r in np.random.default_rng([seed, zlib.crc32(L.name.encode())]).permutation(n_rows)]


def relayout(ss, layout, seed=0, odd_row=None):
    """`ss` on another layout: span_row_start, row_base, row_ncells and
    row_val_len are the same arrays; the offsets and the byte buffers are new,
    every row's bytes copied unchanged and wholly inside the buffers. odd_row:
    the row the one_off_* layouts move (default: the middle one)."""
    L = LAYOUTS[layout] if isinstance(layout, str) else layout
    if L.name == "packed":
        return ss
    R = ss.n_rows
    qlen = 2 * ss.row_ncells.astype(np.int64)
    vlen = ss.row_val_len.astype(np.int64)
    odd = (R // 2 if odd_row is None else int(odd_row)) if L.odd else -1
    order = row_order(R, L, seed)
    if L.q is None:
        qoff = (np.cumsum(qlen) - qlen).astype(np.uint64)
        qend = int(qlen.sum())
    else:
        qoff, qend = _place(order, qlen, L.q, Q_UNIT, odd if L.odd == "q" else -1, 2)
    if L.v is None:
        voff = (np.cumsum(vlen) - vlen + np.arange(R)).astype(np.uint64)
        vend = int(voff[-1]) + int(vlen[-1]) if R else 0
    else:
        voff, vend = _place(order, vlen, L.v, V_UNIT, odd if L.odd == "v" else -1, 8)
    qb = np.full(qend + TAIL, L.fill, np.uint8)
    vb = np.full(vend + TAIL, L.fill, np.uint8)
    for r in range(R):
        q0, v0 = int(ss.row_qual_off[r]), int(ss.row_val_off[r])
        qb[int(qoff[r]):int(qoff[r]) + int(qlen[r])] = ss.qual_bytes[q0:q0 + int(qlen[r])]
        vb[int(voff[r]):int(voff[r]) + int(vlen[r])] = ss.val_bytes[v0:v0 + int(vlen[r])]
    return packing.SpanSet(ss.span_row_start, ss.row_base, ss.row_ncells, qoff, voff, ss.row_val_len, qb, vb)


def extents(ss):
    """(qualifier, value) bytes up to the end of the last row in each buffer"""
    if not ss.n_rows:
        return 0, 0
    return (int((ss.row_qual_off.astype(np.int64) + 2 * ss.row_ncells.astype(np.int64)).max()),
            int((ss.row_val_off.astype(np.int64) + ss.row_val_len.astype(np.int64)).max()))


def outside_rows(ss):
    """(qualifier, value) boolean masks of the bytes no row holds"""
    qm, vm = np.ones(len(ss.qual_bytes), bool), np.ones(len(ss.val_bytes), bool)
    for r in range(ss.n_rows):
        qo, vo = int(ss.row_qual_off[r]), int(ss.row_val_off[r])
        qm[qo:qo + 2 * int(ss.row_ncells[r])] = False
        vm[vo:vo + int(ss.row_val_len[r])] = False
    return qm, vm


def cell_width(ss, r):
    """W of a compacted row of one width (0: none)"""
    n, vl = int(ss.row_ncells[r]), int(ss.row_val_len[r])
    vb = vl - 1 if n > 1 else vl
    return vb // n if n and vb % n == 0 else 0


# ---- the kernels' membership predicates, restated on a SpanSet ----

def rows_streamable(ss):
    """every row at 8 B (qualifiers) and 16 B (values): reg_rows_ok, k_ug_ds_reg's
    first row and dir_fields (k_ds_reg.hip), k_ds_spans (k_ds_chunks.hip)"""
    return bool(((ss.row_qual_off & np.uint64(7)) == 0).all() and ((ss.row_val_off & np.uint64(15)) == 0).all())


def rows_proposable(ss):
    """every span's first row at an even qualifier offset and a value offset
    that is a multiple of its cell width: ug_probe (k_assemble.hip), ls_probe
    (k_direct.hip)"""
    for s in range(ss.n_spans):
        r = int(ss.span_row_start[s])
        W = cell_width(ss, r)
        if W not in (4, 8) or int(ss.row_qual_off[r]) & 1 or int(ss.row_val_off[r]) & (W - 1):
            return False
    return True
