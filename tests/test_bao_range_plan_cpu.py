"""The rows of the range planner without a GPU (b3w_sample_rows_ranges, bao.sample_rows_ranges): the closed form for a range's rows held
against b3w_sample_rows_batch over bao.runs_chunks of the same ranges, and the per-chunk provable flags against b3w_chain_path_provable
chunk by chunk.  Files and ranges: the 51 lengths and the range kinds of tests/test_bao_range_cpu.py (_long_ranges, and every single chunk
of the files of at most 70 chunks)."""
import numpy as np
import pytest

import b3w_testlib as T
from test_bao_range_cpu import ALL_LENGTHS, _long_ranges

BAD = 100
SHORT = 70


def _ranges(length):
    n = max(1, (length + 1023) // 1024)
    return _long_ranges(n) + ([(c, 1) for c in range(n)] if n <= SHORT else [])


def test_names_and_the_abi_version():
    m = T.pkg()
    L = m.lib()
    assert L.b3w_abi_version() == (1 << 16) | 4                            # new names only
    header = open(T.ROOT + "/include/b3wit.h").read() if hasattr(T, "ROOT") else None
    for name in ("b3w_sample_rows_ranges", "b3w_sample_plan_range_slices_device"):
        assert name in m.EXPORTED_SYMBOLS and hasattr(L, name)
        assert header is None or name + "(" in header
    for name in ("sample_rows_ranges", "plan_samples_range_slices", "prove_samples_range_slices"):
        assert callable(getattr(m.bao, name))


@pytest.mark.parametrize("length", ALL_LENGTHS)
def test_rows_are_sample_rows_batch_over_runs_chunks(length):
    m = T.pkg()
    L = m.lib()
    ranges = _ranges(length)
    order = np.random.default_rng(length + 5).permutation(len(ranges))      # any order, and one range twice
    first = np.array([ranges[i][0] for i in order] + [ranges[0][0]], dtype=np.uint64)
    count = np.array([ranges[i][1] for i in order] + [ranges[0][1]], dtype=np.uint64)
    lens = np.array([3 * 1024 + 1, length], dtype=np.uint64)                # the file is not the batch's first
    files = np.ones(first.size, dtype=np.uint32)
    rrf, crf, provable = m.bao.sample_rows_ranges(lens, files, first, count)
    c_files, chunks = m.bao.runs_chunks(files, first, count)
    want = m.bao.sample_rows_batch(lens, c_files, chunks)
    chunk_first = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    assert np.array_equal(crf, want), length
    assert np.array_equal(rrf, want[chunk_first]), length                   # (the last entry of both is the total)
    assert int(rrf[-1]) == int(want[-1]) == int(crf[-1])
    n = max(1, (length + 1023) // 1024)
    assert provable.dtype == bool and provable.size == chunks.size
    assert provable.tolist() == [bool(L.b3w_chain_path_provable(int(c), n)) for c in chunks], length


def test_a_batch_of_files_and_the_null_optional_outputs():
    m = T.pkg()
    L = m.lib()
    lens = np.array([5 * 1024 + 7, 0, 70 * 1024, 1, 2049 * 1024], dtype=np.uint64)
    files = np.array([0, 2, 1, 2, 0, 3, 4, 4, 4], dtype=np.uint32)
    first = np.array([1, 3, 0, 69, 5, 0, 0, 1023, 2048], dtype=np.uint64)
    count = np.array([3, 64, 1, 1, 1, 1, 2049, 1026, 1], dtype=np.uint64)
    rrf, crf, provable = m.bao.sample_rows_ranges(lens, files, first, count)
    c_files, chunks = m.bao.runs_chunks(files, first, count)
    want = m.bao.sample_rows_batch(lens, c_files, chunks)
    assert np.array_equal(crf, want) and np.array_equal(rrf, want[np.concatenate([[0], np.cumsum(count)]).astype(np.int64)])
    total = int(count.sum())
    args = (lens.ctypes.data, lens.size, files.ctypes.data, first.ctypes.data, count.ctypes.data, count.size)
    # each optional output alone, and neither: the same totals, the other array untouched
    r2 = np.full(count.size + 1, 77, dtype=np.uint64)
    assert L.b3w_sample_rows_ranges(*args, r2.ctypes.data, None, None) == int(want[-1]) and np.array_equal(r2, rrf)
    c2 = np.full(total + 1, 77, dtype=np.uint64)
    assert L.b3w_sample_rows_ranges(*args, r2.ctypes.data, c2.ctypes.data, None) == int(want[-1]) and np.array_equal(c2, want)
    p2 = np.full(total, 77, dtype=np.uint8)
    assert L.b3w_sample_rows_ranges(*args, r2.ctypes.data, None, p2.ctypes.data) == int(want[-1]) and np.array_equal(p2.astype(bool), provable)
    assert set(p2.tolist()) <= {0, 1}
    # no range at all
    r0 = np.full(1, 77, dtype=np.uint64)
    assert L.b3w_sample_rows_ranges(None, 0, None, None, None, 0, r0.ctypes.data, None, None) == 0 and int(r0[0]) == 0
    empty = m.bao.sample_rows_ranges(lens, [], [], [])
    assert empty[0].tolist() == [0] and empty[1].tolist() == [0] and empty[2].size == 0


def test_a_whole_gib_file_is_counted_without_a_walk_over_its_chunks():
    m = T.pkg()
    L = m.lib()
    lens = np.array([1 << 30, (5 << 30) + 300], dtype=np.uint64)
    files = np.array([0, 1, 1], dtype=np.uint32)
    first = np.array([0, (1 << 22) - 3, 5 * (1 << 20) - 1], dtype=np.uint64)
    count = np.array([1 << 20, 7, 2], dtype=np.uint64)
    rrf = np.zeros(4, dtype=np.uint64)
    total = L.b3w_sample_rows_ranges(lens.ctypes.data, 2, files.ctypes.data, first.ctypes.data, count.ctypes.data, 3, rrf.ctypes.data, None, None)
    assert int(rrf[1]) == (1 << 20) * (16 + 20) == 37748736                # a full tree of 2^20 chunks: sixteen blocks and twenty nodes a chunk
    c_files, chunks = m.bao.runs_chunks(files[1:], first[1:], count[1:])
    want = m.bao.sample_rows_batch(lens, c_files, chunks)
    assert total == int(rrf[3]) == int(rrf[1]) + int(want[-1]) and int(rrf[2]) - int(rrf[1]) == int(want[7])


def test_refusals_leave_the_outputs_untouched():
    m = T.pkg()
    L = m.lib()
    lens = np.array([5 * 1024 + 7, 0, 70 * 1024], dtype=np.uint64)
    for f, a, k in ((3, 0, 1), (0, 0, 0), (0, 5, 2), (0, 6, 1), (1, 1, 1), (1, 0, 2), (2, 2, 2 ** 64 - 1)):   # a bad file, an empty range, past the end
        files = np.array([2, f], dtype=np.uint32)
        first = np.array([0, a], dtype=np.uint64)
        count = np.array([70, k], dtype=np.uint64)
        rrf = np.full(3, 77, dtype=np.uint64)
        crf = np.full(80, 77, dtype=np.uint64)
        prov = np.full(80, 77, dtype=np.uint8)
        got = L.b3w_sample_rows_ranges(lens.ctypes.data, 3, files.ctypes.data, first.ctypes.data, count.ctypes.data, 2, rrf.ctypes.data, crf.ctypes.data,
                                       prov.ctypes.data)
        assert got == -BAD, (f, a, k)
        assert (rrf == 77).all() and (crf == 77).all() and (prov == 77).all(), (f, a, k)
        with pytest.raises(m.B3WError):
            m.bao.sample_rows_ranges(lens, files, first, count)
    one = np.zeros(1, dtype=np.uint64)
    files = np.zeros(1, dtype=np.uint32)
    count = np.ones(1, dtype=np.uint64)
    rrf = np.zeros(2, dtype=np.uint64)
    assert L.b3w_sample_rows_ranges(lens.ctypes.data, 3, files.ctypes.data, one.ctypes.data, count.ctypes.data, 1, None, None, None) == -BAD
    assert L.b3w_sample_rows_ranges(None, 3, files.ctypes.data, one.ctypes.data, count.ctypes.data, 1, rrf.ctypes.data, None, None) == -BAD
    assert L.b3w_sample_rows_ranges(lens.ctypes.data, 3, files.ctypes.data, one.ctypes.data, None, 1, rrf.ctypes.data, None, None) == -BAD
    assert L.b3w_sample_rows_ranges(lens.ctypes.data, 3, files.ctypes.data, one.ctypes.data, count.ctypes.data, 1, rrf.ctypes.data, None, None) == 16 + 3
