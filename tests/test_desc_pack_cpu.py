"""core.pack_offsets, the host restatement of tsdbhip_desc_pack's placement
rule (include/tsdbhip.h), pinned against packing.pack_spans: the same
offsets and the same buffer lengths for the same rows, so that the GPU tests
of test_desc_pack.py compare the kernel against one rule stated twice."""
import numpy as np
import pytest

from opentsdb_amd import core, packing


def random_spans(seed, n_spans, max_rows, max_cells):
    """rows of 0..max_cells cells of 1..8 value bytes each (+ the meta byte of
    a compacted row of several cells); some spans empty"""
    rng = np.random.default_rng(seed)
    spans = []
    for _ in range(n_spans):
        rows = []
        for _ in range(int(rng.integers(0, max_rows + 1))):
            n = int(rng.integers(0, max_cells + 1))
            w = int(rng.integers(1, 9))
            vl = n * w + (1 if n > 1 else 0)
            rows.append(packing.KeyValue(int(rng.integers(0, 1 << 32)), rng.bytes(2 * n), rng.bytes(vl)))
        spans.append(rows)
    return spans


def check(spans):
    ss = packing.pack_spans(spans)
    qoff, voff, qn, vn = core.pack_offsets(ss.row_ncells, ss.row_val_len)
    assert qoff.dtype == np.uint64 and voff.dtype == np.uint64
    np.testing.assert_array_equal(qoff, ss.row_qual_off)
    np.testing.assert_array_equal(voff, ss.row_val_off)
    assert (qn, vn) == (len(ss.qual_bytes), len(ss.val_bytes))


@pytest.mark.parametrize("seed", range(8))
def test_offsets_equal_the_packers_on_random_rows(seed):
    check(random_spans(seed, 1 + 5 * seed, 4, 40 if seed % 2 else 700))


def test_zero_length_rows_zero_rows_and_empty_spans():
    kv = packing.KeyValue
    check([])                                            # no span: buffers of 16 zero bytes
    check([[], [], []])                                  # spans without rows
    check([[kv(0, b"", b"")]])                           # one row of nothing
    check([[kv(0, b"", b""), kv(3600, b"\x00\x07", b"\x01" * 8)], [], [kv(0, b"", b"")]])
    check([[kv(0, b"\x00\x07", b"\x01" * 8)], [kv(0, b"", b"")], []])  # the last rows add nothing to the length
    # lengths at the alignment edges: 7, 8 and 9 qualifier pairs; 15, 16 and 17 value bytes
    check([[kv(0, b"\x00\x01" * n, b"\x05" * v)] for n, v in ((3, 15), (4, 16), (5, 17), (4, 15), (1, 1))])


def test_offsets_are_computed_in_64_bits():
    """150,000 rows of 3600 eight-byte cells put the last offsets above 2^32"""
    n = 150_000
    qoff, voff, qn, vn = core.pack_offsets(np.full(n, 3600, np.uint32), np.full(n, 28801, np.uint32))
    assert int(voff[-1]) == 28816 * (n - 1) > 1 << 32 and vn == 28816 * n
    assert int(qoff[-1]) == 7200 * (n - 1) and qn == 7200 * n
