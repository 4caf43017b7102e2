"""core.quals_proven, the host restatement of tsdbhip_desc_certify, on
hand-built rows (cert_cases.py): what TSDBHIP_DESC_QUALS_PROVEN states of a
row, checked without a GPU. tests/test_values_only_certificate.py holds the kernel to this
function."""
import numpy as np
import pytest

import cert_cases as cc
from opentsdb_amd import core, packing

ROWS = cc.hand_rows()


@pytest.mark.parametrize("name,words,proven", ROWS, ids=[r[0] for r in ROWS])
def test_row(name, words, proven):
    assert core.row_quals_proven(np.asarray(words, ">u2").tobytes()) == proven
    # ... and as the middle row of a table, between proven neighbours
    ok = core.quals_proven(cc.table([cc.quals(9), words, cc.quals(600, 1, 3)]))
    assert ok.tolist() == [True, proven, True]


def test_every_place_is_covered():
    """the unproven hand rows change cell 1, cell 2, a middle cell and the last
    cell, in the flags nibble (float flag, width 4, an illegal width) and in
    the delta"""
    names = [r[0] for r in ROWS]
    for what in list(cc.FLAGS) + list(cc.DELTA):
        for c in (1, 2, 10, 19):
            assert f"{what} at cell {c} of 20" in names


def test_the_statement_is_about_the_bytes_only():
    """float cells and 4-byte integers on one step are proven rows: the cell
    type is the query's business"""
    assert core.row_quals_proven(np.asarray(cc.quals(100, 0, 7, flags=0x3), ">u2").tobytes())
    assert core.row_quals_proven(np.asarray(cc.quals(100, 0, 7, flags=0xF), ">u2").tobytes())


def test_rows_outside_the_buffer_or_at_an_odd_offset():
    ss = cc.table([cc.quals(30), cc.quals(1), cc.quals(30)])
    assert core.quals_proven(ss).all()
    qn = int(ss.row_qual_off[2]) + 60
    assert core.quals_proven(ss, qn).all()
    assert core.quals_proven(ss, qn - 1).tolist() == [True, True, False]
    off = ss.row_qual_off.copy()
    off[1] += np.uint64(1)  # (a one-cell row: proven whatever its bytes, were it at an even offset)
    odd = packing.SpanSet(ss.span_row_start, ss.row_base, ss.row_ncells, off, ss.row_val_off, ss.row_val_len,
                          ss.qual_bytes, ss.val_bytes)
    assert core.quals_proven(odd).tolist() == [True, False, True]


def test_empty_table():
    ss = packing.pack_spans([])
    assert len(core.quals_proven(ss)) == 0
