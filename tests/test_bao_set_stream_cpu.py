"""Set slices taken in windows, without a GPU: the names, argument lists and constants of the session calls, and the host call
b3w_bao_set_slice_stream_cuts (bao.set_slice_cuts) with b3w_bao_set_slice_stream_scratch_bytes against the restatement in
tests/bao_set_stream_ref.py - the cuts read off bao_set_ref.encode's emission order (offset and c0 of every element) and the greedy
window plan.  Files: test_bao_range_cpu's 51 lengths, every shape of test_bao_set_cpu.set_shapes, the empty file, and the fabricated
5 GiB + 300 B file of test_gpu_bao_set (from the host call alone)."""
import ctypes
import os
import re

import numpy as np
import pytest

import b3w_testlib as T
import bao_set_stream_ref as SR
from test_bao_range_cpu import ALL_LENGTHS
from test_bao_set_cpu import set_shapes

BAD = 100
MIN = 8 + 64 * (24 + 1023) + 1048576
CARRY = 1552
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"b3w_bao_set_slice_stream_cuts": 7, "b3w_bao_set_slice_stream_scratch_bytes": 5, "b3w_bao_set_slice_stream_begin": 19,
         "b3w_bao_set_slice_stream_push": 5, "b3w_bao_set_slice_stream_finish": 1, "b3w_bao_set_slice_stream_free": 1}
WINDOWS = (MIN, 2 * MIN, 1 << 40)                          # the least window, twice that, larger than any slice here


def _u64(x):
    return np.array(x, dtype=np.uint64)


def _raw_cuts(L, length, runs, window, cap=None):
    """the C call with an exact-size list -> (the return value, the list)"""
    fc, nc = _u64([a for a, _ in runs]), _u64([k for _, k in runs])
    k = L.b3w_bao_set_slice_stream_cuts(length, fc.ctypes.data, nc.ctypes.data, fc.size, window, None, 0)
    if k < 0:
        return k, None
    out = np.full((k + 1) if cap is None else cap, 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
    assert L.b3w_bao_set_slice_stream_cuts(length, fc.ctypes.data, nc.ctypes.data, fc.size, window, out.ctypes.data if out.size else None, out.size) == k
    return k, out


def _most_rows(cuts, window):
    """the most rows a window of at most `window` bytes holds, wherever it starts"""
    best, j = 0, 0
    for i in range(len(cuts) - 1):
        j = max(j, i + 1)
        while j < len(cuts) - 1 and cuts[j + 1] - cuts[i] <= window:
            j += 1
        best = max(best, j - i)
    return best


def _check(m, length, runs, what):
    L = m.lib()
    first, count = [a for a, _ in runs], [k for _, k in runs]
    cuts, B = SR.row_cuts(length, runs)
    size = m.bao.set_slice_size(length, first, count)
    assert cuts[0] == 0 and cuts[-1] == size, what
    assert all(b > a for a, b in zip(cuts, cuts[1:])) and all(c % 16 == 8 for c in cuts[1:-1]), what
    assert max(b - a for a, b in zip(cuts, cuts[1:])) <= MIN, what
    # a row of the table per cut: the receiver's scratch counts the same rows
    ln, fi, fc, nc = _u64([length]), np.zeros(len(runs), dtype=np.uint32), _u64(first), _u64(count)
    rows = L.b3w_bao_set_slice_ingest_scratch_bytes(ln.ctypes.data, 1, fi.ctypes.data, fc.ctypes.data, nc.ctypes.data, len(runs)) // 16
    assert rows == len(cuts) - 1, what
    for window in WINDOWS:
        want = SR.greedy(cuts, window)
        got = m.bao.set_slice_cuts(length, first, count, window)
        assert got.dtype == np.uint64 and got.tolist() == want, (what, window)
        assert int(got[-1]) == size and all(int(c) % 16 == 8 for c in got[1:-1]), (what, window)
        k, short = _raw_cuts(L, length, runs, window, cap=len(want) - 1)       # one too small: the count, nothing written
        assert k == len(want) - 1 and (short == 0xEEEEEEEEEEEEEEEE).all(), (what, window)
        assert L.b3w_bao_set_slice_stream_scratch_bytes(length, fc.ctypes.data, nc.ctypes.data, fc.size, window) == CARRY + 16 * _most_rows(cuts, window), (what, window)
    if cuts[-1] > MIN:
        assert len(SR.greedy(cuts, MIN)) > 2, what                              # (the least window does cut such a slice)
    return cuts, B


@pytest.mark.parametrize("length", ALL_LENGTHS)
def test_the_cuts_against_the_restatement(length):
    m = T.pkg()
    n = m.bao.num_chunks(length)
    for name, runs in set_shapes(n).items():
        _check(m, length, runs, (length, name))


def test_more_rows_than_one_window_and_the_empty_file():
    m = T.pkg()
    assert _check(m, 0, [(0, 1)], "the empty file") == ([0, 8], 64)
    # 3 MiB + 5 and 5 MiB + 300: several tiles under a ragged upper tree, sparse and dense rows
    seen = set()
    for length in (3 * (1 << 20) + 5, 5 * (1 << 20) + 300):
        n = m.bao.num_chunks(length)
        for name, runs in set_shapes(n).items():
            cuts, B = _check(m, length, runs, (length, name))
            seen.add((B, len(cuts) - 1))
    assert {b for b, _ in seen} == {64, 1024} and max(r for _, r in seen) == 6


def test_names_argument_lists_constant_and_rust_declarations():
    m = T.pkg()
    L = m.lib()
    assert L.b3w_abi_version() == (1 << 16) | 4                            # new names only
    header = open(os.path.join(ROOT, "include", "b3wit.h")).read()
    rust = open(os.path.join(ROOT, "integrations", "rust", "b3wit_ffi.rs")).read()
    for name, n_args in NAMES.items():
        assert name in m.EXPORTED_SYMBOLS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == n_args, name
        decl = re.search(re.escape(name) + r"\(([^;{]*?)\);", header, re.S).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == n_args, name
        rs = re.search(r"pub fn " + re.escape(name) + r"\((.*?)\)", rust, re.S).group(1)
        assert len(rs.split(",")) == n_args, name
    assert f"#define B3W_BAO_SET_SLICE_STREAM_MIN_WINDOW {MIN}ull" in header and f"#define B3W_BAO_SET_SLICE_STREAM_CARRY_BYTES {CARRY}ull" in header
    assert m.bao.SET_SLICE_STREAM_MIN_WINDOW == MIN == SR.MIN_WINDOW and m.bao.SET_SLICE_STREAM_CARRY_BYTES == CARRY
    assert (m.bao.SET_STREAM_ARENA, m.bao.SET_STREAM_PACKED) == (0, 1)
    assert "#define B3W_BAO_SET_STREAM_ARENA  0" in header and "#define B3W_BAO_SET_STREAM_PACKED 1" in header
    assert m.bao.DEFAULT_SET_SLICE_WINDOW_BYTES >= MIN
    for name in ("set_slice_cuts", "SetSliceStream", "ingest_set_slice_stream"):
        assert callable(getattr(m.bao, name))
    for name in ("push", "finish", "close"):
        assert callable(getattr(m.bao.SetSliceStream, name))


def test_the_cuts_of_a_file_of_5_gib():
    """test_gpu_bao_set's fabricated file and runs: a chunk in the first tile, a run across chunk 2^22 (file byte 2^32), the ragged last
    chunk - four rows of 1 024, from the host call alone and from the walk over the four paths"""
    m = T.pkg()
    length = (5 << 30) + 300
    n = m.bao.num_chunks(length)
    runs = [(7, 1), ((1 << 22) - 1, 3), (n - 1, 1)]
    cuts, B = _check(m, length, runs, "5 GiB + 300 B")
    assert B == 1024 and len(cuts) == 5
    # the places, said aloud: a row's cut is the end of the wanted chunk before its block
    first, count = [a for a, _ in runs], [k for _, k in runs]
    assert cuts[1] == 8 + 64 * 23 + 1024                                       # chunk 7's path: the root over 2^22 | the rest, then 22 whole levels
    assert cuts[2] == cuts[1] + 64 * 21 + 1024                                 # chunk 2^22 - 1 parts from chunk 7 at the node over [0, 2^22): 21 below it
    assert cuts[4] == m.bao.set_slice_size(length, first, count)
    assert cuts[4] - cuts[3] <= 64 * 24 + 300


def test_refusals_that_need_no_device():
    m = T.pkg()
    L = m.lib()
    length = 5 * 1024 + 7
    guard = np.full(8, 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
    good = (_u64([1, 4]), _u64([2, 2]))

    def cuts(length=length, fc=good[0], nc=good[1], k=2, window=MIN, out=guard, cap=8):
        return L.b3w_bao_set_slice_stream_cuts(length, fc.ctypes.data if fc is not None else None, nc.ctypes.data if nc is not None else None, k, window,
                                               out.ctypes.data if out is not None else None, cap)

    def scratch(length=length, fc=good[0], nc=good[1], k=2, window=MIN, **_):
        return L.b3w_bao_set_slice_stream_scratch_bytes(length, fc.ctypes.data if fc is not None else None, nc.ctypes.data if nc is not None else None, k, window)
    for kw in (dict(k=0), dict(fc=None), dict(nc=None), dict(fc=_u64([4, 1])), dict(fc=_u64([1, 2])), dict(nc=_u64([2, 0])), dict(nc=_u64([2, 3])),
               dict(fc=_u64([1, 6])), dict(window=MIN - 1), dict(window=0), dict(length=(1 << 40) + 1025, fc=_u64([0, 4]))):
        assert cuts(**kw) == -BAD, kw
        assert (guard == 0xEEEEEEEEEEEEEEEE).all(), kw
        assert scratch(**kw) == 0, kw
        with pytest.raises(m.B3WError):
            m.bao.set_slice_cuts(kw.get("length", length), [] if kw.get("k") == 0 else kw.get("fc", good[0]) if kw.get("fc", 1) is not None else [],
                                 [] if kw.get("k") == 0 else kw.get("nc", good[1]) if kw.get("nc", 1) is not None else [], kw.get("window", MIN))
    assert cuts(out=None, cap=0) == 1 and cuts(cap=1) == 1 and (guard == 0xEEEEEEEEEEEEEEEE).all()
    assert cuts(cap=2) == 1 and guard.tolist()[:3] == [0, m.bao.set_slice_size(length, [1, 4], [2, 2]), 0xEEEEEEEEEEEEEEEE]
    assert scratch() == CARRY + 16
    # the session calls without a session or a context
    assert L.b3w_bao_set_slice_stream_push(None, 0, None, 0, None) == BAD
    assert L.b3w_bao_set_slice_stream_finish(None) == BAD
    L.b3w_bao_set_slice_stream_free(None)
    h = ctypes.c_void_p(77)
    assert L.b3w_bao_set_slice_stream_begin(None, length, 0, good[0].ctypes.data, good[1].ctypes.data, 2, None, 0, None, 0, None, None, None, None, None, None, 0,
                                            None, ctypes.byref(h)) == BAD and h.value == 77
